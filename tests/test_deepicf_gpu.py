"""DeepICF on the device (csrc/deepicf.hip, neurec_amd/deepicf.py) against the reference class's own trace
(tests/golden/tfgraph_deepicf*.npz) and the float64 restatement (tests/deepicf_restatement.py).

The bar against the trace is the project's standing one: 4 x the reference's own float32-to-float64 gap of that
variable and step plus 1e-5 max|want|.  Only the pre-norm biases under batch norm are left out of the per-variable
comparison (the reference's float32 run moves them by Adam-amplified rounding noise, the device writes exact zeros);
predict() covers them.  Against the restatement (shapes the trace does not hold) the bar is 2e-5 max|want|: float32's
6e-8, times the batch norm's 1 / sqrt(epsilon) = 32 at worst, times sqrt(128) = 11 for a sum over the widest layer."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import deepicf_restatement as D
from test_deepicf_cpu import STEP_CASES
from test_fism_gpu import _toy
from test_gru4rec_gpu import _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return D.load_trace(load_golden)


def _make(R, T, hy, max_batch, **kw):
    from neurec_amd.deepicf import DeepICFEngine
    L = len(hy["layers"])
    tower = {k: T[k] for k in ["Wout", "bout"] + ["W%d" % i for i in range(L)] + ["b%d" % i for i in range(L)]}
    if hy["batch_norm"]:
        tower.update({k + str(i): T[k + str(i)] for k in ("beta", "gamma", "mm", "mv") for i in range(L)})
    act = hy["activation"] if hy["activation"] in (0, 1, 2) else "Relu"
    kw.setdefault("learner", hy.get("learner", "adam"))
    return DeepICFEngine(T["c1"], T["Q"], T["W"], T["b"], tower, R, kw.pop("lr", hy.get("lr", 0.01)), hy["regs"],
                         hy["regw"], hy["alpha"], hy["beta"], max_batch, algorithm=hy["algorithm"], activation=act,
                         batch_norm=bool(hy["batch_norm"]), bias=T["bias"], h=T["h"], **kw)


def _engine(g, case, **kw):
    hy = D.golden_hyper(g, case)
    return _make(D.golden_matrix(g, case), D.golden_init(g, case), hy, 16, **kw), hy


def _feed(eng, users, items, labels, loss2):
    import torch
    dev = eng.c1.device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    eng.step(t(users, torch.int32), t(items, torch.int32), t(labels, torch.float32), loss2)
    return loss2


def _vars(eng):
    out = {k: getattr(eng, k).cpu().numpy().astype(np.float64) for k in eng._names}
    for i, (m, v) in enumerate(zip(eng.mm, eng.mv)):
        out["mm%d" % i], out["mv%d" % i] = m.cpu().numpy().astype(np.float64), v.cpu().numpy().astype(np.float64)
    return out


def _pre_norm(name, hy):
    return bool(hy["batch_norm"]) and re.fullmatch(r"b\d+", name) is not None


def _compare_tables(g, case, eng, hy, init, step):
    for name, got in _vars(eng).items():
        want = D.golden_var(g, case, init, name, step).reshape(got.shape)
        if _pre_norm(name, hy):
            assert np.array_equal(got, init[name].astype(np.float64).reshape(got.shape)), name      # exact zeros
            continue
        err, tol = np.abs(got - want).max(), D.tolerance(g, case, name, step, want)
        print("%s step %d %s: device err %.3g, bar %.3g" % (case, step + 1, name, err, tol))
        assert err <= tol, (case, step, name, err, tol)


def _loss_ok(g, case, k, got):
    want, ref32 = float(g[case + "_loss_f64"][k]), float(g[case + "_loss_f32"][k])
    print("%s step %d loss: device err %.3g, reference f32 err %.3g" % (case, k + 1, abs(got - want), abs(ref32 - want)))
    return abs(got - want) <= 4 * abs(ref32 - want) + 1e-5 * abs(want)


@pytest.mark.parametrize("case", STEP_CASES)
def test_steps_match_the_reference_trace(golden, case):
    """every loss and every variable, moving statistics included, after every step"""
    import torch
    g = golden
    eng, hy = _engine(g, case)
    init = D.golden_init(g, case)
    loss2 = torch.zeros(2, device=eng.c1.device)
    for k, (users, items, labels) in enumerate(D.golden_batches(g, case)):
        _feed(eng, users, items, labels, loss2)
        assert _loss_ok(g, case, k, float(loss2.cpu().numpy().astype(np.float64).sum()))
        _compare_tables(g, case, eng, hy, init, k)


def _score_bar(g, name):
    want = g[name + "_f64"]
    return want, 4 * np.abs(g[name + "_f32"].astype(np.float64) - want).max() + 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("pair_kernel", ["mfma", "valu"])
def test_score_matches_the_reference_predict(golden, pair_kernel):
    """predict() after the last step of `default`, full and candidate mode, on both scorer paths; score() leaves the
    moving statistics and every table as they are, and twice is bit-identical"""
    import torch
    g = golden
    eng, hy = _engine(g, "default", pair_kernel=pair_kernel)
    assert eng.tower_mfma == (pair_kernel == "mfma")
    loss2 = torch.zeros(2, device=eng.c1.device)
    for users, items, labels in D.golden_batches(g, "default"):
        _feed(eng, users, items, labels, loss2)
    before = _vars(eng)
    got = eng.score(g["predict_users"]).cpu().numpy()
    again = eng.score(g["predict_users"]).cpu().numpy()
    assert np.array_equal(got, again)
    after = _vars(eng)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    want, bar = _score_bar(g, "predict_default")
    err = np.abs(got - want).max()
    print("predict (%s): device err %.3g, bar %.3g" % (pair_kernel, err, bar))
    assert err <= bar
    cand = np.take_along_axis(got, g["predict_cand"].astype(np.int64), axis=1)
    want, bar = _score_bar(g, "predict_default_cand")
    assert np.abs(cand - want).max() <= bar


@pytest.fixture(scope="module")
def epoch_run(golden):
    """the recorded train_model() epoch on the device: (losses [steps], the end variables, predict() after it)"""
    import torch
    g = golden
    eng, hy = _engine(g, "epoch")
    batches = D.golden_batches(g, "epoch")
    losses = torch.zeros((len(batches), 2), device=eng.c1.device)
    for k, (users, items, labels) in enumerate(batches):
        _feed(eng, users, items, labels, losses[k])
    eng.verify()
    return losses.cpu().numpy().astype(np.float64).sum(axis=1), _vars(eng), eng.score(g["predict_users"]).cpu().numpy()


def test_epoch_matches_the_reference_trace(golden, epoch_run):
    """369 steps of 16 (the last partial) as the class fed them: every loss, the end variables, predict() after it"""
    g = golden
    losses, got, scores = epoch_run
    hy, init = D.golden_hyper(g, "epoch"), D.golden_init(g, "epoch")
    assert len(losses) == len(g["epoch_sizes"]) and np.isfinite(losses).all()
    for k, loss in enumerate(losses):
        assert _loss_ok(g, "epoch", k, loss), k
    for name, have in got.items():
        if _pre_norm(name, hy):
            assert np.array_equal(have, init[name].astype(np.float64).reshape(have.shape))
            continue
        want = D.golden_var(g, "epoch", init, name, 0).reshape(have.shape)
        err, tol = np.abs(have - want).max(), D.tolerance(g, "epoch", name, 0, want)
        print("epoch %s: device err %.3g, bar %.3g" % (name, err, tol))
        assert err <= tol, (name, err, tol)
    want, bar = _score_bar(g, "predict_epoch")
    err = np.abs(scores - want).max()
    print("predict after the epoch: device err %.3g, bar %.3g" % (err, bar))
    assert err <= bar


def test_two_epochs_end_bit_identical(golden, epoch_run):
    import torch
    g = golden
    eng, _ = _engine(g, "epoch")
    batches = D.golden_batches(g, "epoch")
    losses = torch.zeros((len(batches), 2), device=eng.c1.device)
    for k, (users, items, labels) in enumerate(batches):
        _feed(eng, users, items, labels, losses[k])
    first_losses, first, first_scores = epoch_run
    assert np.array_equal(losses.cpu().numpy().astype(np.float64).sum(axis=1), first_losses)
    second = _vars(eng)
    assert all(np.array_equal(first[k], second[k]) for k in first)
    assert np.array_equal(eng.score(g["predict_users"]).cpu().numpy(), first_scores)


# ------------------------------------------------------------------ against the restatement
def _random_hyper(d, w, layers, algorithm, activation, batch_norm, learner="gd", lr=0.05):
    return dict(algorithm=algorithm, activation=activation, alpha=0.5, beta=0.5, layers=list(layers),
                batch_norm=int(batch_norm), regs=[0.01, 0.02, 0.001], regw=[0.5] * len(layers), d=d, w=w,
                learner=learner, lr=lr)


def _tables(I, hy, seed):
    T = D.init_tables(I, hy["d"], hy["w"], hy["layers"], hy["algorithm"], hy["batch_norm"], seed)
    rs = np.random.RandomState(seed + 1)
    for k, n in enumerate(hy["layers"] if hy["batch_norm"] else []):
        T["mm%d" % k] = (0.3 * rs.randn(n)).astype(np.float32)
        T["mv%d" % k] = (0.5 + rs.rand(n)).astype(np.float32)
    return T


SCORE_SHAPES = [(16, 16, [64, 32, 16], 0, -1, "mfma"), (16, 16, [64, 32, 16], 1, -1, "mfma"),
                (16, 16, [64, 32, 16], 0, 2, "valu"), (20, 9, [96, 24], 1, 0, "auto"), (40, 16, [33], 0, 1, "mfma"),
                (7, 5, [12, 5], 1, 2, "valu"), (64, 16, [64, 64, 64, 64], 0, -1, "mfma")]


@pytest.mark.parametrize("d,w,layers,algorithm,activation,pair_kernel", SCORE_SHAPES)
def test_score_against_the_restatement(d, w, layers, algorithm, activation, pair_kernel):
    """both scorer paths and both algorithms, one and two 32-tiles of width, a width only the fallback takes, a packed
    tower beyond the 48 KB staged in LDS (four layers of 64 at d = 64: the matrix-core kernel reads it from memory);
    77 items
    (no multiple of the 32-item tile), 11 users (more than the 8 of a workgroup), a user without history, a user
    whose history is every item but one, and a user outside the matrix"""
    import scipy.sparse as sp
    rs = np.random.RandomState(d + 7)
    U, I = 14, 77
    rows, cols = [], []
    for u in range(U):
        deg = {0: 0, 1: I - 1, 2: 1}.get(u, int(rs.randint(2, 30)))
        rows += [u] * deg
        cols += sorted(rs.choice(I, deg, replace=False).tolist())
    R = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(U, I))
    hy = _random_hyper(d, w, layers, algorithm, activation, True)
    T = _tables(I, hy, 40 + d)
    eng = _make(R, T, hy, 8, pair_kernel=pair_kernel)
    assert eng.tower_mfma == (pair_kernel == "mfma")
    users = np.asarray([0, 1, 2, 5, 3, 9, 13, 4, 1, 7, 11], np.int32)
    want = D.predict(R, T, hy, users)
    got = eng.score(users).cpu().numpy()
    err = np.abs(got - want).max()
    print("score d=%d layers=%s alg=%d %s: err %.3g" % (d, layers, algorithm, pair_kernel, err))
    assert err <= 2e-5 * np.abs(want).max()
    assert np.array_equal(got, eng.score(users).cpu().numpy())
    outside = eng.score(np.asarray([U + 3, 0], np.int32)).cpu().numpy()
    assert np.array_equal(outside[0], outside[1]) and np.array_equal(outside[1], got[0])      # both pool nothing


def _batch(R, B, rs, short=False):
    """short: histories of at most 4 items beside one of 70, so that nearly every instance carries the padding row and
    it weighs in its softmax sum"""
    deg = np.diff(R.indptr)
    users = rs.choice(np.flatnonzero((deg > 0) & (deg < (5 if short else 80))), B)
    if short:
        users[0] = 3
    items, labels = [], []
    for k, u in enumerate(users):
        row = R.indices[R.indptr[u]:R.indptr[u + 1]]
        if k % 2 == 0:
            items.append(int(row[rs.randint(len(row))]))
            labels.append(1.0)
        else:
            items.append(int(R.shape[1] - 1 - rs.randint(5)))
            labels.append(0.0)
    return users.astype(np.int32), np.asarray(items, np.int32), np.asarray(labels, np.float32)


@pytest.mark.parametrize("B,batch_norm,mask", [(33, True, "reference"), (70, True, "reference"), (1, True, "reference"),
                                               (2, True, "reference"), (33, False, "reference"),
                                               (33, True, "history"), (5, False, "history")])
def test_one_step_against_the_restatement(B, batch_norm, mask):
    """the batch statistics across two and three row tiles of 32 (33 and 70 rows), batches of 1 and 2, and the tower
    without batch norm: every variable and the moving statistics after one step of plain gradient descent (the update
    is linear in the gradient, so a wrong term shows at its full size); under both attention masks, and the two masks
    give different tables on the same batch"""
    import torch
    R = _toy()
    hy = _random_hyper(16, 16, [40, 24], 1, 2, batch_norm)
    T = _tables(R.shape[1], hy, 300 + B)
    eng = _make(R, T, hy, 70, attention_mask=mask)
    assert eng.reference_mask == (mask == "reference")
    users, items, labels = _batch(R, B, np.random.RandomState(B), short=mask == "history")
    st = D.State(T, hy, learner="gd", lr=hy["lr"])
    want_loss = D.step(st, R, users, items, labels, mask=mask)
    if mask == "history":
        other = D.State(T, hy, learner="gd", lr=hy["lr"])
        D.step(other, R, users, items, labels, mask="reference")
        assert np.abs(other.var["c1"] - st.var["c1"]).max() > 50 * 2e-5 * np.abs(st.var["c1"]).max()
    loss2 = _feed(eng, users, items, labels, torch.zeros(2, device=eng.c1.device))
    got_loss = float(loss2.cpu().numpy().astype(np.float64).sum())
    assert abs(got_loss - want_loss) <= 2e-5 * abs(want_loss)
    for name, got in _vars(eng).items():
        want = st.var[name].reshape(got.shape)
        err = np.abs(got - want).max()
        print("B=%d bn=%d %s: err %.3g of %.3g" % (B, batch_norm, name, err, np.abs(want).max()))
        assert err <= 2e-5 * max(np.abs(want).max(), 1e-3), (name, err)


def test_bessel_keyword_and_dense_q_keyword():
    """`bessel=False` moves the moving variance without the correction; `q_application` reaches HistoryEngine"""
    import torch
    R = _toy()
    hy = _random_hyper(16, 16, [24], 0, -1, True)
    T = _tables(R.shape[1], hy, 77)
    users, items, labels = _batch(R, 5, np.random.RandomState(3))
    ends = {}
    for bessel in (True, False):
        eng = _make(R, T, hy, 8, bessel=bessel)
        assert eng.q_dense and eng.flag_Q is None
        _feed(eng, users, items, labels, torch.zeros(2, device=eng.c1.device))
        st = D.State(T, hy, learner="gd", lr=hy["lr"])
        D.step(st, R, users, items, labels, bessel=bessel)
        ends[bessel] = eng.mv[0].cpu().numpy().astype(np.float64)
        assert np.abs(ends[bessel] - st.var["mv0"]).max() <= 2e-5 * np.abs(st.var["mv0"]).max()
    assert np.abs(ends[True] - ends[False]).max() > 1e-3
    with pytest.raises(ValueError, match="q_application"):
        _make(R, T, hy, 8, q_application="sparse")


# ------------------------------------------------------------------ drop-in
def _metrics(line):
    return np.asarray([float(x) for x in line.split()])


def test_deepicf_config_drops_in(tmp_path):
    """NeuRec.properties + conf/DeepICF.properties (the reference's values) on ml-100k: two epochs through
    neurec_amd.main; the reference's log lines, a finite falling loss, metrics above the untrained model's"""
    untrained = _run(tmp_path / "untrained", ["--recommender=DeepICF", "--epochs=0"])
    base = _metrics(untrained.evaluate())
    model = _run(tmp_path, ["--recommender=DeepICF", "--epochs=2"])
    eng = model.engine
    assert (eng.d, eng.w, eng.layers, eng.algorithm, eng.activation, eng.batch_norm, eng.max_batch, eng.learner) == \
        (16, 16, [64, 32, 16], 1, 3, True, 256, "adam")
    assert eng.regw == [10.0, 10.0, 0.0] and eng.q_dense and eng.reference_mask
    folder = os.path.join(str(tmp_path), "log", "ml-100k", "DeepICF")
    files = os.listdir(folder)
    assert len(files) == 1
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "DeepICF's hyperparameters:" in text and "load pretrained params unsuccessful!" in text
    lines = [ln for ln in text.splitlines()
             if re.search(r"metrics:\t|\[iter \d+ : loss : [0-9.]+, time: [0-9.]+\]|epoch \d+:\t", ln)]
    kinds = [("m" if "metrics:" in ln else "i%s" % re.search(r"iter (\d+)", ln).group(1)
              if "[iter" in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)) for ln in lines]
    assert kinds == ["m", "i1", "e1", "i2", "e2"], kinds
    losses = [float(x) for x in re.findall(r"\[iter \d+ : loss : ([0-9.]+), time", text)]
    assert np.all(np.isfinite(losses)) and losses[1] < losses[0]
    trained = _metrics(re.findall(r"epoch 2:\t(.+)", text)[0])
    print("untrained", base, "trained", trained)
    assert np.all(np.isfinite(trained)) and np.all(trained > base)
    full = model.predict([0, 5, 9], None)
    assert tuple(full.shape) == (3, model.num_items) and full.is_cuda and bool(full.isfinite().all())
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full.cpu().numpy()[0][[1, 2, 3]])


def test_limits_and_refusals(tmp_path, monkeypatch):
    R = _toy()
    I = R.shape[1]
    hy = _random_hyper(16, 16, [8, 8, 8, 8, 8], 0, -1, True)
    with pytest.raises(NotImplementedError, match="5 layers"):
        _make(R, _tables(I, hy, 1), hy, 8)
    hy = _random_hyper(16, 16, [129], 0, -1, True)
    with pytest.raises(NotImplementedError, match="width 129"):
        _make(R, _tables(I, hy, 1), hy, 8)
    hy = _random_hyper(16, 16, [96], 0, -1, True)
    with pytest.raises(NotImplementedError, match="matrix-core"):
        _make(R, _tables(I, hy, 1), hy, 8, pair_kernel="mfma")
    with pytest.raises(NotImplementedError, match="layers"):
        _run(tmp_path / "a", ["--recommender=DeepICF", "--epochs=1", "--layers=[8,8,8,8,8]"])
    with pytest.raises(NotImplementedError, match="width"):
        _run(tmp_path / "b", ["--recommender=DeepICF", "--epochs=1", "--layers=[200,8]"])
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)                                # WORLD_SIZE > 1
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(tmp_path / "c", ["--recommender=DeepICF", "--epochs=1"])
