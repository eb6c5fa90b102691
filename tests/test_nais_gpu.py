"""NAIS on the GPU (csrc/nais.hip through neurec_amd/nais.py): every step of the reference class's trace, predict() for
both algorithms, the edge shapes against the restatement, determinism, the drop-in run through neurec_amd.main and the
refusals."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from neurec_amd import defaults
import fism_restatement as F
import nais_restatement as NA
from test_nais_cpu import CASES
from test_fism_gpu import _pointwise_batch, _toy, _with_slots_that_take_no_part, _write_dataset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return NA.load_trace(load_golden)


def _engine(g, case, **kw):
    from neurec_amd.nais import NAISEngine
    loss, learner, pairwise = CASES[case]
    hy = NA.golden_hyper(g, case)
    return NAISEngine(g["c1_0"], g["Q0"], g["W0_a%d" % hy["algorithm"]], g["b_0"], F.golden_matrix(g),
                      float(g["learning_rate"]), g["regs"], hy["alpha"], hy["beta"], 64, algorithm=hy["algorithm"],
                      activation=hy["activation"], loss=loss, pairwise=pairwise, learner=learner, bias=g["bias_0"],
                      h=g["h_0"], **kw)


def _feed(eng, users, items, third, loss2):
    import torch
    dev = eng.c1.device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    eng.step(t(users, torch.int32), t(items, torch.int32), t(third, torch.int32 if eng.pairwise else torch.float32),
             loss2)
    return float(loss2.cpu().numpy().astype(np.float64).sum())


def _tables(eng):
    return [getattr(eng, k).cpu().numpy() for k in NA.NAMES]


def _run_case(g, eng, case):
    import torch
    loss2 = torch.zeros(2, device=eng.c1.device)
    return [_feed(eng, g[case + "_users"][k], g[case + "_items"][k], g[case + "_third"][k], loss2)
            for k in range(len(g[case + "_users"]))]


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Tables (c1, Q, bias, W, b, h) and loss after every step against the f64 trace: within 4x the reference's own
    f32-to-f64 distance of that step and table plus the floor 1e-5 max|want| (test_fism_gpu.py's bar).  The measured
    ratios are printed; DESIGN.md 6e quotes them."""
    import torch
    g = golden
    eng = _engine(g, case)
    loss2 = torch.zeros(2, device=eng.c1.device)
    for k in range(len(g[case + "_users"])):
        loss = _feed(eng, g[case + "_users"][k], g[case + "_items"][k], g[case + "_third"][k], loss2)
        want, ref32 = g[case + "_f64_loss"][k], g[case + "_f32_loss"][k]
        print("%s step %d loss: device err %.3g, reference f32 err %.3g" % (case, k + 1, abs(loss - want),
                                                                           abs(ref32 - want)))
        assert abs(loss - want) <= 4 * abs(ref32 - want) + 1e-5 * abs(want)
        for name, got, w64, w32 in zip(NA.NAMES, _tables(eng), NA.golden_tables(g, case, "f64", k),
                                       NA.golden_tables(g, case, "f32", k)):
            bar = np.abs(w32.astype(np.float64) - w64).max()
            err = np.abs(got.astype(np.float64) - w64).max()
            print("%s step %d %s: device err %.3g, reference f32 err %.3g, ratio %.2f"
                  % (case, k + 1, name, err, bar, err / bar if bar else float("inf") if err else 0.0))
            assert err <= 4 * bar + 1e-5 * np.abs(w64).max(), (case, k, name, err, bar)


@pytest.mark.parametrize("case", ["a0_none_ce", "a1_tanh"])
def test_score_matches_the_reference_predict(golden, case):
    """score() after the trained case against predict()'s trace (the 1,100-item user included), the empty-row user,
    and candidate mode's entries"""
    g = golden
    R = F.golden_matrix(g)
    users = g["predict_users"]
    eng = _engine(g, case)
    _run_case(g, eng, case)
    a = NA.golden_hyper(g, case)["algorithm"]
    w64, w32 = g["predict_a%d_f64" % a], g["predict_a%d_f32" % a].astype(np.float64)
    got = eng.score(users).cpu().numpy().astype(np.float64)
    bar, err = np.abs(w32 - w64).max(), np.abs(got - w64).max()
    print("predict %s: device err %.3g, reference f32 err %.3g, ratio %.2f" % (case, err, bar, err / bar))
    assert got.shape == w64.shape and err <= 4 * bar + 1e-5 * np.abs(w64).max()
    empty = int(np.flatnonzero(np.diff(R.indptr) == 0)[0])
    mixed = eng.score(np.asarray([empty, int(users[1])], np.int32)).cpu().numpy()
    assert np.array_equal(mixed[0], eng.bias.cpu().numpy())
    assert np.array_equal(mixed[1], eng.score(users[1:2]).cpu().numpy()[0])       # a row does not depend on its block
    from neurec_amd.model.general_recommender.NAIS import NAIS
    plugin = NAIS.__new__(NAIS)
    plugin.engine = eng
    full = plugin.predict(users.tolist(), None).cpu().numpy()
    cand = plugin.predict(users.tolist()[:2], [[3, 0, 1199], [7]])
    assert np.array_equal(cand[0], full[0][[3, 0, 1199]]) and np.array_equal(cand[1], full[1][[7]])


def _tables_for(I, d, w, algorithm, rs):
    f = lambda x: x.astype(np.float32)
    rows = (algorithm + 1) * d
    sign = np.where(rs.rand(w) < 0.5, -1.0, 1.0)
    return (f(0.2 * rs.randn(I, d)), f(0.2 * rs.randn(I, d)), f(0.01 * rs.randn(I)),
            f(rs.randn(rows, w) / np.sqrt(rows)), f(sign * (0.3 + 0.2 * rs.rand(w))), f((1.0 + 0.3 * rs.randn(w)) / np.sqrt(w)))


def _check_against_restatement(eng, T, R, batches, loss, pairwise, hy, mask, learner="gd", lr=0.2, c1_rows=False,
                               restated=None):
    """device tables after every batch within 4x the restatement's own f32-to-f64 distance + 1e-5 max|want|;
    restated: the batches the restatement gets where they are not the engine's"""
    import torch
    regs = [0.01, 0.02]
    s64 = NA.State(*T, learner=learner, lr=lr)
    s32 = NA.State(*T, learner=learner, lr=lr, dtype=np.float32)
    loss2 = torch.zeros(2, device=eng.c1.device)
    for fed, (users, items, third) in zip(batches, restated or batches):
        got = _feed(eng, *fed, loss2)
        want = NA.step(s64, R, users, items, third, pairwise, loss, regs, mask=mask, c1_rows=c1_rows, **hy)
        w32 = NA.step(s32, R, users, items, third, pairwise, loss, regs, mask=mask, c1_rows=c1_rows, **hy)
        assert abs(got - want) <= 4 * abs(w32 - want) + 1e-5 * abs(want), (got, want, w32)
        for name, t in zip(NA.NAMES, _tables(eng)):
            bar = np.abs(s32.var[name].astype(np.float64) - s64.var[name]).max()
            err = np.abs(t.astype(np.float64) - s64.var[name]).max()
            assert err <= 4 * bar + 1e-5 * np.abs(s64.var[name]).max(), (name, len(users), err, bar)
    return s64


# relu is left to the trace (whose maker keeps every pre-activation away from the kink): here f32 and f64 could
# disagree on the side of a kink
EDGES = [(1, 1, (33,), 0.5, 0, "reference", -1), (16, 16, (1,), 0.5, 0, "reference", 2),
         (16, 16, (64, 64, 17), 0.5, 0, "reference", 2), (16, 16, (64, 64, 17), 1.0, 1, "history", 1),
         (20, 24, (33,), 1.0, 1, "reference", 1), (64, 64, (33,), 0.0, 0, "history", 2),
         (128, 16, (33,), 0.5, 1, "history", -1), (128, 64, (33,), 0.5, 0, "reference", 1),
         (16, 1, (33,), 0.0, 1, "reference", 2), (64, 24, (33,), 1.0, 0, "reference", -1)]


@pytest.mark.parametrize("d,w,batches,beta,algorithm,mask,activation", EDGES)
def test_edges_against_the_restatement(d, w, batches, beta, algorithm, mask, activation):
    """every lane layout (w = 1, 16, 24, 64 columns; d = 1, 16, 20, 64, 128), B = 1, a short last batch, beta 0 / 0.5 / 1,
    both algorithms and both mask forms on histories of 0 to 257 rows; plain gradient descent with a large step, so a
    wrong or missing term of any gradient shows at its full size; then score() of every user"""
    from neurec_amd.nais import NAISEngine
    R = _toy()
    rs = np.random.RandomState(1000 * d + w)
    T = _tables_for(R.shape[1], d, w, algorithm, rs)
    hy = dict(algorithm=algorithm, activation=activation, alpha=0.5, beta=beta)
    # beta = 0 leaves the sum of exp() unnormalised: outputs and gradients are some hundred times larger, and the step
    # that keeps the tables finite is that much smaller
    lr = 0.02 if beta > 0 else 1e-4
    eng = NAISEngine(T[0], T[1], T[3], T[4], R, lr, [0.01, 0.02], 0.5, beta, max(batches), algorithm=algorithm,
                     activation=activation, loss="square", learner="gd", bias=T[2], h=T[5], attention_mask=mask)
    st = _check_against_restatement(eng, T, R, [_pointwise_batch(R, B, rs) for B in batches], "square", False, hy, mask,
                                    lr=lr)
    users = np.arange(R.shape[0], dtype=np.int32)
    dev = [t.astype(np.float64) for t in _tables(eng)]
    want = NA.predict(R, dev, users, **hy)
    import torch
    w32 = NA.predict(R, dev, users, dtype=torch.float32, **hy)
    got = eng.score(users).cpu().numpy()
    assert np.abs(got - want).max() <= 4 * np.abs(w32 - want).max() + 1e-5 * np.abs(want).max()
    assert st is not None


@pytest.mark.parametrize("learner", ["momentum", "adam"])
def test_c1_by_rows_option(learner):
    """c1_application="rows": c1 gets the sparse application on the rows the batch's histories hold, against the
    restatement of that form under the same bar (Adam included: the f32 restatement carries Adam's own amplification
    of rounding, so the bar scales with it); two steps, so that a row of step 1 alone is swept (Adam) or left (momentum)"""
    from neurec_amd.nais import NAISEngine
    R = _toy()
    rs = np.random.RandomState(11)
    T = _tables_for(R.shape[1], 16, 16, 0, rs)
    hy = dict(algorithm=0, activation=2, alpha=0.5, beta=0.5)
    lr = 0.01 if learner == "adam" else 0.05
    eng = NAISEngine(T[0], T[1], T[3], T[4], R, lr, [0.01, 0.02], 0.5, 0.5, 40, activation=2, loss="square",
                     learner=learner, bias=T[2], h=T[5], c1_application="rows")
    batches = [_pointwise_batch(R, 40, rs) for _ in range(2)]
    _check_against_restatement(eng, T, R, batches, "square", False, hy, "reference", learner=learner, lr=lr,
                               c1_rows=True)


@pytest.mark.parametrize("pairwise", [False, True])
def test_slots_that_take_no_part(pairwise):
    """a user or an item that is no table row (pairwise also: a user with one train item) takes its slot, or its whole
    pair, out of the step — the side's longest history, the padding term, included: two gd steps against the
    restatement fed the same batches without those slots, under the edge shapes' bar.  Square loss (pairwise: bpr): a
    sum over the instances — the pointwise cross-entropy is a mean over the batch's length, every slot included"""
    from neurec_amd.nais import NAISEngine
    R = _toy()
    rs = np.random.RandomState(31)
    T = _tables_for(R.shape[1], 16, 16, 0, rs)
    hy = dict(algorithm=0, activation=2, alpha=0.5, beta=0.5)
    loss = "bpr" if pairwise else "square"
    eng = NAISEngine(T[0], T[1], T[3], T[4], R, 0.02, [0.01, 0.02], 0.5, 0.5, 33, algorithm=0, activation=2,
                     loss=loss, pairwise=pairwise, learner="gd", bias=T[2], h=T[5], attention_mask="reference")
    both = [_with_slots_that_take_no_part(R, rs, pairwise) for _ in range(2)]
    _check_against_restatement(eng, T, R, [fed for fed, _ in both], loss, pairwise, hy, "reference", lr=0.02,
                               restated=[kept for _, kept in both])
    eng.verify()


def test_gradient_buffer_follows_the_batch():
    """the ragged [positions, d] buffer holds the batch's history positions, not B x the longest row: it grows to what
    a batch takes, and a caller's too-small `positions` is an error, not a silently dropped gradient"""
    import torch
    from neurec_amd.nais import NAISEngine
    R = _toy()
    rs = np.random.RandomState(2)
    T = _tables_for(R.shape[1], 16, 16, 0, rs)
    deg = np.diff(R.indptr)
    mk = lambda: NAISEngine(T[0], T[1], T[3], T[4], R, 0.01, [0.01, 0.02], 0.5, 0.5, 40, activation=2, loss="square",
                            learner="gd", bias=T[2], h=T[5])
    eng = mk()
    assert eng.row_cap < 40 * int(deg.max())
    loss2 = torch.zeros(2, device=eng.c1.device)
    batch = _pointwise_batch(R, 40, rs)
    _feed(eng, *batch, loss2)
    need = int(deg[batch[0]].sum())
    assert int(eng.positions(torch.from_numpy(batch[0]).to(eng.c1.device))) == need
    assert need <= eng.row_cap < 40 * int(deg.max()) and int(eng._need[0]) == need
    eng.verify()
    small = mk()
    dev = small.c1.device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    small.row_cap, small._rows = 8, torch.empty((8, 16), device=dev)
    small.step(t(batch[0], torch.int32), t(batch[1], torch.int32), t(batch[2], torch.float32), loss2, positions=8)
    with pytest.raises(RuntimeError, match="history positions"):
        small.verify()


def test_empty_histories_and_equal_lengths():
    """a batch whose histories are all empty (width 0: out = bias[i], only Q's regulariser and the bias move) and a
    batch whose histories all have one length (no padding term anywhere: both mask forms give the same bytes)"""
    import torch
    from neurec_amd.nais import NAISEngine
    R = _toy()
    rs = np.random.RandomState(5)
    T = _tables_for(R.shape[1], 16, 16, 1, rs)
    hy = dict(algorithm=1, activation=2, alpha=0.5, beta=0.5)
    mk = lambda mask: NAISEngine(T[0], T[1], T[3], T[4], R, 0.2, [0.01, 0.02], 0.5, 0.5, 8, algorithm=1, activation=2,
                                 loss="square", learner="gd", bias=T[2], h=T[5], attention_mask=mask)
    deg = np.diff(R.indptr)
    one = int(np.flatnonzero(deg == 1)[0])
    item = int(R.indices[R.indptr[one]])
    empty = (np.asarray([one, one], np.int32), np.asarray([item, item], np.int32), np.ones(2, np.float32))
    eng = mk("reference")
    _check_against_restatement(eng, T, R, [empty], "square", False, hy, "reference")
    got = _tables(eng)
    assert all(np.array_equal(got[j], T[j]) for j in (0, 3, 4, 5)) and not np.array_equal(got[2], T[2])
    same = np.flatnonzero(deg == np.bincount(deg[deg > 2]).argmax())[:4].astype(np.int32)
    assert len(same) >= 2
    batch = (same, np.full(len(same), R.shape[1] - 1, np.int32), np.zeros(len(same), np.float32))
    a, b = mk("reference"), mk("history")
    _check_against_restatement(a, T, R, [batch], "square", False, hy, "reference")
    loss2 = torch.zeros(2, device=b.c1.device)
    _feed(b, *batch, loss2)
    assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in NA.NAMES)


@pytest.mark.parametrize("case", ["a0_none_ce", "bpr"])
def test_two_engines_end_byte_identical(golden, case):
    import torch
    g = golden
    out = []
    for _ in range(2):
        eng = _engine(g, case)
        losses = _run_case(g, eng, case)
        out.append([getattr(eng, k).clone() for k in NA.NAMES] + [eng.score(g["predict_users"]).clone(), losses])
    assert all(torch.equal(a, b) for a, b in zip(out[0][:7], out[1][:7])) and out[0][7] == out[1][7]


@pytest.mark.parametrize("case", ["a0_none_ce", "a1_tanh", "bpr"])
def test_key_sort_path_matches_the_reference_trace(golden, case):
    """c1_path="sort": G_c1 from the sorted (item | position) keys instead of the walk, under the trace's bar (the
    1,100-item history, a user twice, excluded first / last are in these batches); the two paths sum in different
    fixed orders, so they are compared with the trace, not with each other bit for bit"""
    import torch
    g = golden
    eng = _engine(g, case, c1_path="sort")
    loss2 = torch.zeros(2, device=eng.c1.device)
    for k in range(len(g[case + "_users"])):
        _feed(eng, g[case + "_users"][k], g[case + "_items"][k], g[case + "_third"][k], loss2)
        for name, got, w64, w32 in zip(NA.NAMES, _tables(eng), NA.golden_tables(g, case, "f64", k),
                                       NA.golden_tables(g, case, "f32", k)):
            bar = np.abs(w32.astype(np.float64) - w64).max()
            err = np.abs(got.astype(np.float64) - w64).max()
            assert err <= 4 * bar + 1e-5 * np.abs(w64).max(), (case, k, name, err, bar)
    eng.verify()
    again = _engine(g, case, c1_path="sort")
    _run_case(g, again, case)
    assert all(torch.equal(getattr(eng, k), getattr(again, k)) for k in NA.NAMES)


def test_key_sort_path_wide_rows():
    """the sort path at d = 128 (two columns per lane) and a short last batch, against the restatement"""
    from neurec_amd.nais import NAISEngine
    R = _toy()
    rs = np.random.RandomState(77)
    T = _tables_for(R.shape[1], 128, 16, 1, rs)
    hy = dict(algorithm=1, activation=2, alpha=0.5, beta=0.5)
    eng = NAISEngine(T[0], T[1], T[3], T[4], R, 0.02, [0.01, 0.02], 0.5, 0.5, 40, algorithm=1, activation=2,
                     loss="square", learner="gd", bias=T[2], h=T[5], c1_path="sort")
    _check_against_restatement(eng, T, R, [_pointwise_batch(R, B, rs) for B in (40, 9)], "square", False, hy,
                               "reference", lr=0.02)


@pytest.mark.parametrize("case", ["a0_none_ce", "a0_relu_square", "a0_sigmoid_b1"])
def test_matrix_core_pair_kernel(golden, case):
    """pair_kernel="mfma": score() through v_mfma_f32_16x16x4f32 against predict()'s trace (case a0_none_ce) and
    against the VALU kernel (every activation): both are fp32 chains of the same terms in another order, so they
    agree to a few ulp of the largest score, not bit for bit"""
    g = golden
    users = g["predict_users"]
    valu, mfma = _engine(g, case, pair_kernel="valu"), _engine(g, case, pair_kernel="mfma")
    assert mfma.mfma and not valu.mfma
    _run_case(g, valu, case)
    _run_case(g, mfma, case)
    a, b = valu.score(users).cpu().numpy().astype(np.float64), mfma.score(users).cpu().numpy().astype(np.float64)
    assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max()
    if case == "a0_none_ce":
        w64, w32 = g["predict_a0_f64"], g["predict_a0_f32"].astype(np.float64)
        bar, err = np.abs(w32 - w64).max(), np.abs(b - w64).max()
        print("predict mfma: device err %.3g, reference f32 err %.3g, ratio %.2f" % (err, bar, err / bar))
        assert err <= 4 * bar + 1e-5 * np.abs(w64).max()
    empty = int(np.flatnonzero(np.diff(F.golden_matrix(g).indptr) == 0)[0])
    assert np.array_equal(mfma.score(np.asarray([empty], np.int32)).cpu().numpy()[0], mfma.bias.cpu().numpy())
    with pytest.raises(NotImplementedError, match="matrix-core"):
        _engine(g, "a1_tanh", pair_kernel="mfma")


# ------------------------------------------------------------------ drop-in
NAIS_PROPERTIES = """[hyperparameters]
pretrain=1
verbose=1
learner=adam
batch_size=256
epochs=100
weight_size=16
embedding_size=16
data_alpha=0
regs=[1e-7,1e-7,1e-5]
alpha=0
beta=0.5
num_neg=4
learning_rate=0.001
activation=Relu
algorithm=0
is_pairwise=False
loss_function=cross_entropy
embed_init_method=tnormal
weight_init_method=he_normal
stddev=0.01
pretrain_file=None
"""


def _run(tmp_path, argv):
    from neurec_amd.main import main
    path = defaults.write_default_configs(str(tmp_path), overrides={
        "data.input.path": os.path.join(str(tmp_path), "dataset"), "data.input.dataset": "toy",
        "test_batch_size": "64"})
    with open(os.path.join(str(tmp_path), "conf", "NAIS.properties"), "w") as f:
        f.write(NAIS_PROPERTIES)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return main(argv=argv, properties=path)
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("pairwise", [False, True])
def test_nais_config_drops_in(tmp_path, pairwise):
    _write_dataset(str(tmp_path))
    argv = ["--recommender=NAIS", "--epochs=2"] + (["--is_pairwise=True", "--loss_function=bpr"] if pairwise else [])
    model = _run(tmp_path, argv)
    folder = os.path.join(str(tmp_path), "log", "toy", "NAIS")
    files = os.listdir(folder)
    assert len(files) == 1 and files[0].startswith("toy_NAIS_")
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "NAIS's hyperparameters:" in text
    assert "load pretrained params unsuccessful!" in text
    assert "activation: none (activation='Relu' is not 0, 1 or 2)" in text
    assert "attention mask: reference" in text
    assert ("pairwise structure: positive side = history without the item" in text) == pairwise
    lines = [ln for ln in text.splitlines()
             if re.search(r"metrics:\t|\[iter \d+ : loss : [0-9.]+, time: [0-9.]+\]|epoch \d+:\t", ln)]
    kinds = [("m" if "metrics:" in ln else "i%s" % re.search(r"iter (\d+)", ln).group(1)
              if "[iter" in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)) for ln in lines]
    assert kinds == ["m", "i1", "e1", "i2", "e2"], kinds
    evals = re.findall(r"epoch (\d+):\t(.+)", text)
    vals = [float(x) for x in re.findall(r"[-+]?\d*\.\d+(?:[eE][-+]?\d+)?", evals[-1][1])]
    assert vals and np.all(np.isfinite(vals))
    full = model.predict([0, 5, 9], None)
    assert tuple(full.shape) == (3, model.num_items) and bool(full.isfinite().all())
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full.cpu().numpy()[0][[1, 2, 3]])


def test_history_mask_drops_in(tmp_path):
    _write_dataset(str(tmp_path))
    model = _run(tmp_path, ["--recommender=NAIS", "--epochs=1", "--attention_mask=history", "--activation=2"])
    assert model.engine.reference_mask is False and model.engine.activation == 2


def test_refusals(tmp_path, monkeypatch):
    from neurec_amd.nais import NAISEngine
    R = _toy()
    z = lambda *s: np.zeros(s, np.float32)
    I = R.shape[1]
    with pytest.raises(NotImplementedError, match="128"):
        NAISEngine(z(I, 129), z(I, 129), z(129, 16), z(16), R, 0.01, [0.0, 0.0], 0.0, 0.5, 8)
    with pytest.raises(NotImplementedError, match="64"):
        NAISEngine(z(I, 16), z(I, 16), z(16, 65), z(65), R, 0.01, [0.0, 0.0], 0.0, 0.5, 8)
    with pytest.raises(ValueError, match="beta"):
        NAISEngine(z(I, 16), z(I, 16), z(16, 16), z(16), R, 0.01, [0.0, 0.0], 0.0, -0.5, 8)
    _write_dataset(str(tmp_path))
    with pytest.raises(NotImplementedError):
        _run(tmp_path, ["--recommender=NAIS", "--epochs=1", "--embedding_size=129"])
    with pytest.raises(NotImplementedError):
        _run(tmp_path, ["--recommender=NAIS", "--epochs=1", "--weight_size=65"])
    with pytest.raises(ValueError, match="beta"):
        _run(tmp_path, ["--recommender=NAIS", "--epochs=1", "--beta=-1"])
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)                                # WORLD_SIZE > 1
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(tmp_path, ["--recommender=NAIS", "--epochs=1"])
