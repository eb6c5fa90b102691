"""FISM on the GPU (csrc/fism.hip through neurec_amd/fism.py): every step of the reference class's trace, predict(),
dense versus row application, the edge shapes against the float64 restatement, determinism, the drop-in run through
neurec_amd.main and the refusals."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_golden
from neurec_amd import defaults
import fism_restatement as F
from test_fism_cpu import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_fism")


def _engine(g, case=None, alpha=None, **kw):
    from neurec_amd.fism import FISMEngine
    loss, learner, pairwise = CASES[case] if case else ("square", "adam", False)
    return FISMEngine(g["c1_0"], g["Q0"], F.golden_matrix(g), float(g["learning_rate"]), g["regs"],
                      float(g["alpha"]) if alpha is None else alpha, 64, loss=loss, pairwise=pairwise, learner=learner,
                      bias=g["bias_0"], **kw)


def _feed(eng, users, items, third, loss2):
    import torch
    dev = eng.c1.device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    eng.step(t(users, torch.int32), t(items, torch.int32), t(third, torch.int32 if eng.pairwise else torch.float32),
             loss2)
    return float(loss2.cpu().numpy().astype(np.float64).sum())


def _tables(eng):
    return [t.cpu().numpy() for t in (eng.c1, eng.Q, eng.bias)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Tables and loss after every step against the f64 trace: within 4x the reference's own f32-to-f64 distance of
    that step and table (a different, fixed summation order over histories of up to 1,100 rows), plus the floor
    1e-5 max|want|.  Measured ratios (device error / reference f32 error): see DESIGN.md 6d."""
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
        for name, got, w64, w32 in zip(("c1", "Q", "bias"), _tables(eng), F.golden_tables(g, case, "f64", k),
                                       F.golden_tables(g, case, "f32", k)):
            bar = np.abs(w32.astype(np.float64) - w64).max()
            err = np.abs(got.astype(np.float64) - w64).max()
            print("%s step %d %s: device err %.3g, reference f32 err %.3g, ratio %.2f"
                  % (case, k + 1, name, err, bar, err / bar if bar else float("inf") if err else 0.0))
            assert err <= 4 * bar + 1e-5 * np.abs(w64).max(), (case, k, name, err, bar)


def test_predict_matches_the_reference(golden):
    """full and candidate mode after the trained case, alpha = 0 on the initial tables, and the empty-row user"""
    import torch
    g = golden
    R = F.golden_matrix(g)
    users = g["predict_users"]
    eng = _engine(g, "square_adam")
    loss2 = torch.zeros(2, device=eng.c1.device)
    case = "square_adam"
    for k in range(len(g[case + "_users"])):
        _feed(eng, g[case + "_users"][k], g[case + "_items"][k], g[case + "_third"][k], loss2)
    empty = int(np.flatnonzero(np.diff(R.indptr) == 0)[0])
    for e, w64, w32 in ((eng, g["predict_f64"], g["predict_f32"]),
                        (_engine(g, alpha=0.0), g["predict0_f64"], g["predict0_f32"])):
        got = e.score(users).cpu().numpy().astype(np.float64)
        bar, err = np.abs(w32 - w64).max(), np.abs(got - w64).max()
        print("predict alpha=%g: device err %.3g, reference f32 err %.3g" % (e.alpha, err, bar))
        assert got.shape == w64.shape and err <= 4 * bar + 1e-5 * np.abs(w64).max()
        assert np.array_equal(e.score(np.asarray([empty], np.int32)).cpu().numpy()[0], e.bias.cpu().numpy())
    # the plugin's predict(): the same rows through the evaluator's factors; candidate mode = their entries
    from neurec_amd.model.general_recommender._common import predict_scores
    P, Q = eng.eval_factors()
    full = predict_scores(P, Q, users.tolist(), None)
    assert np.abs(full - g["predict_f64"]).max() <= 4 * np.abs(g["predict_f32"] - g["predict_f64"]).max() \
        + 1e-5 * np.abs(g["predict_f64"]).max()
    cand = predict_scores(P, Q, users.tolist()[:2], [[3, 0, 1199], [7]])
    assert np.array_equal(cand[0], full[0][[3, 0, 1199]]) and np.array_equal(cand[1], full[1][[7]])


@pytest.mark.parametrize("case", ["square_momentum", "square_rmsprop"])
def test_dense_c1_and_row_q(golden, case):
    """c1 is applied densely: a row the first batch touched and the second did not still moves (momentum) at step 2,
    as in the trace; a Q row outside the second batch stays where step 1 left it"""
    import torch
    g = golden
    R = F.golden_matrix(g)
    eng = _engine(g, case)
    loss2 = torch.zeros(2, device=eng.c1.device)
    tabs = []
    for k in range(2):
        _feed(eng, g[case + "_users"][k], g[case + "_items"][k], g[case + "_third"][k], loss2)
        tabs.append(_tables(eng))
    hist = [set(np.concatenate([F.history(R, u, e) for u, _, e, _, _ in
                                F.instances(R, g[case + "_users"][k], g[case + "_items"][k], g[case + "_third"][k],
                                            False)]).tolist()) for k in range(2)]
    only1 = sorted(hist[0] - hist[1])
    assert only1
    w1, w2 = F.golden_tables(g, case, "f64", 0)[0], F.golden_tables(g, case, "f64", 1)[0]
    moved_ref = np.abs(w2[only1] - w1[only1]).max(axis=1) > 0
    moved_dev = np.abs(tabs[1][0][only1] - tabs[0][0][only1]).max(axis=1) > 0
    assert np.array_equal(moved_ref, moved_dev)
    if case == "square_momentum":
        assert moved_dev.all()                                # the accumulator keeps pushing the row
    q_only1 = sorted(set(g[case + "_items"][0].tolist()) - set(g[case + "_items"][1].tolist()))
    assert q_only1 and np.array_equal(tabs[1][1][q_only1], tabs[0][1][q_only1])
    assert np.array_equal(tabs[1][2][q_only1], tabs[0][2][q_only1])
    if case == "square_rmsprop":
        # momentum 0: a zero gradient moves no variable under either application, but the dense kernel still decays
        # the row's mean square, ms += (0 - ms) (1 - 0.9), twice from 1; the row kernel leaves an untouched row's at 1
        # (gd and adagrad have nothing that a zero gradient changes: dense and row application coincide for them)
        never_c1 = sorted(set(range(R.shape[1])) - hist[0] - hist[1])
        never_q = sorted(set(range(R.shape[1])) - set(g[case + "_items"][:2].ravel().tolist()))
        ms = np.float32(1.0)
        for _ in range(2):
            ms = np.float32(ms + np.float32(np.float32(0.0 - ms) * np.float32(1.0 - np.float32(0.9))))
        assert never_c1 and never_q
        assert np.all(eng.s0["c1"].cpu().numpy()[never_c1] == ms) and ms < 1
        assert np.all(eng.s0["Q"].cpu().numpy()[never_q] == 1.0)
        assert np.all(eng.s0["bias"].cpu().numpy()[never_q] == 1.0)


@pytest.mark.parametrize("learner", ["momentum", "rmsprop", "adam"])
def test_c1_by_rows_option(learner):
    """c1_application="rows": c1 gets the sparse application on the rows the batch's histories hold, against the
    float64 restatement of that form; two steps, so that a row of step 1 alone stays put at step 2 (momentum)"""
    import torch
    from neurec_amd.fism import FISMEngine
    R = _toy()
    rs = np.random.RandomState(11)
    d = 16
    c1 = (0.1 * rs.randn(R.shape[1], d)).astype(np.float32)
    Q = (0.1 * rs.randn(R.shape[1], d)).astype(np.float32)
    b0 = (0.01 * rs.randn(R.shape[1])).astype(np.float32)
    lr = 0.01 if learner == "adam" else 0.2
    eng = FISMEngine(c1, Q, R, lr, [0.01, 0.02], 0.5, 40, bias=b0, learner=learner, c1_application="rows")
    st = F.State(c1, Q, b0, learner=learner, lr=lr)
    loss2 = torch.zeros(2, device=eng.c1.device)
    prev = None
    for k in range(2):
        users, items, labels = _pointwise_batch(R, 40, rs)
        _feed(eng, users, items, labels, loss2)
        F.step(st, R, users, items, labels, False, "square", 0.5, [0.01, 0.02], c1_rows=True)
        got = _tables(eng)
        if learner != "adam":       # (Adam's g / (|g| + eps) amplifies fp32 rounding near g = 0: the trace covers it)
            for name, t in zip(("c1", "Q", "bias"), got):
                assert np.abs(t - st.var[name]).max() <= 1e-5 * np.abs(st.var[name]).max(), (name, k)
        hist = set(np.concatenate([F.history(R, u, e) for u, _, e, _, _ in
                                   F.instances(R, users, items, labels, False)]).tolist())
        if prev is not None and learner != "adam":
            stay = sorted(prev[1] - hist)
            assert stay and np.array_equal(got[0][stay], prev[0][stay])
        prev = (got[0], hist)
    assert np.all(np.isfinite(_tables(eng)[0]))


@pytest.mark.parametrize("loss", ["hinge", "square", "bpr"])
def test_pairwise_losses_against_the_float64_restatement(loss):
    """every pairwise loss of util/learner.py, two gd steps on pairs that hold one-item users (dropped) and a user
    twice, against the float64 restatement"""
    import torch
    from neurec_amd.fism import FISMEngine
    R = _toy()
    rs = np.random.RandomState(3)
    d = 16
    c1 = (0.3 * rs.randn(R.shape[1], d)).astype(np.float32)
    Q = (0.3 * rs.randn(R.shape[1], d)).astype(np.float32)
    b0 = (0.01 * rs.randn(R.shape[1])).astype(np.float32)
    eng = FISMEngine(c1, Q, R, 0.2, [0.01, 0.02], 0.5, 37, bias=b0, learner="gd", loss=loss, pairwise=True)
    st = F.State(c1, Q, b0, learner="gd", lr=0.2)
    loss2 = torch.zeros(2, device=eng.c1.device)
    for B in (37, 8):
        users, items, _ = _pointwise_batch(R, B, rs)
        items = np.asarray([R.indices[R.indptr[u] + rs.randint(R.indptr[u + 1] - R.indptr[u])] for u in users], np.int32)
        negs = (R.shape[1] - 1 - rs.randint(5, size=B)).astype(np.int32)
        got = _feed(eng, users, items, negs, loss2)
        want = F.step(st, R, users, items, negs, True, loss, 0.5, [0.01, 0.02])
        assert abs(got - want) <= 1e-5 * abs(want), (loss, got, want)
        for name, t in zip(("c1", "Q", "bias"), _tables(eng)):
            assert np.abs(t - st.var[name]).max() <= 1e-5 * np.abs(st.var[name]).max(), (loss, name)


def _toy(n_users=70, n_items=300, seed=5):
    rs = np.random.RandomState(seed)
    rows, cols = [], []
    for u in range(n_users):
        deg = [0, 1, 2, 70, 130, 257][u] if u < 6 else int(rs.randint(1, 40))
        rows += [u] * deg
        cols += rs.choice(n_items - 5, deg, replace=False).tolist()
    R = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_users, n_items))
    R.sort_indices()
    return R


def _pointwise_batch(R, B, rs):
    users = rs.choice(np.flatnonzero(np.diff(R.indptr) > 0), B)
    users[:min(B, 5)] = [1, 2, 3, 4, 5][:min(B, 5)]
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


@pytest.mark.parametrize("d,batches", [(1, (33,)), (16, (1,)), (16, (64, 64, 17)), (20, (40,)), (64, (40,)),
                                       (128, (40, 9))])
def test_edges_against_the_float64_restatement(d, batches):
    """B = 1, a short last batch, every lane layout (d = 1, 16, 20, 64, 128) on histories of 0 to 257 rows, against the
    float64 restatement: 1e-5 max|want| per table (fp32 storage of O(0.1) tables and fp32 loss sums).  The learner is
    plain gradient descent with a large step: the update is linear in the gradient, so a wrong or missing term of any
    gradient shows at its full size (Adam's g / (|g| + eps) hides scale and amplifies rounding near g = 0)"""
    import torch
    from neurec_amd.fism import FISMEngine
    R = _toy()
    rs = np.random.RandomState(d)
    c1 = (0.1 * rs.randn(R.shape[1], d)).astype(np.float32)
    Q = (0.1 * rs.randn(R.shape[1], d)).astype(np.float32)
    b0 = (0.01 * rs.randn(R.shape[1])).astype(np.float32)
    eng = FISMEngine(c1, Q, R, 0.5, [0.01, 0.02], 0.5, max(batches), bias=b0, learner="gd")
    st = F.State(c1, Q, b0, learner="gd", lr=0.5)
    loss2 = torch.zeros(2, device=eng.c1.device)
    for B in batches:
        users, items, labels = _pointwise_batch(R, B, rs)
        got = _feed(eng, users, items, labels, loss2)
        want = F.step(st, R, users, items, labels, False, "square", 0.5, [0.01, 0.02])
        assert abs(got - want) <= 1e-5 * abs(want)
        for name, t in zip(("c1", "Q", "bias"), _tables(eng)):
            err = np.abs(t - st.var[name]).max()
            assert err <= 1e-5 * np.abs(st.var[name]).max(), (name, B, err)
    users = np.arange(R.shape[0], dtype=np.int32)
    want = F.predict(R, *[t.astype(np.float64) for t in _tables(eng)], users, 0.5)
    assert np.abs(eng.score(users).cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()


def _with_slots_that_take_no_part(R, rs, pairwise):
    """(the batch as the engine gets it, the same batch without the slots that take no part): pointwise 33 slots, four
    of them with a user or an item that is no table row; pairwise 17 triples with user 1 (one train item), a negative
    and a positive that are no table rows — before, between and after the slots that count"""
    U, I = R.shape
    if not pairwise:
        users, items, third = _pointwise_batch(R, 33, rs)
        users[0], users[7], items[21], items[32] = -1, U, -1, I
        out = [0, 7, 21, 32]
    else:
        users, _, _ = _pointwise_batch(R, 17, rs)
        items = np.asarray([R.indices[R.indptr[u] + rs.randint(R.indptr[u + 1] - R.indptr[u])] for u in users], np.int32)
        third = (I - 1 - rs.randint(5, size=17)).astype(np.int32)
        assert users[0] == 1 and R.indptr[2] - R.indptr[1] == 1
        third[8], items[16] = I, -1
        out = [0, 8, 16]
    keep = np.setdiff1d(np.arange(len(users)), out)
    return (users, items, third), (users[keep], items[keep], third[keep])


@pytest.mark.parametrize("pairwise", [False, True])
def test_slots_that_take_no_part(pairwise):
    """a user or an item that is no table row (pairwise also: a user with one train item) takes its slot, or its whole
    pair, out of the step: two gd steps give the tables and the loss of the float64 restatement fed the same batches
    without those slots, 1e-5 max|want| as the edge shapes.  Square loss (pairwise: bpr): a sum over the instances —
    the pointwise cross-entropy is a mean over the batch's length, slots that take no part included"""
    import torch
    from neurec_amd.fism import FISMEngine
    R = _toy()
    rs = np.random.RandomState(29)
    d = 16
    c1 = (0.1 * rs.randn(R.shape[1], d)).astype(np.float32)
    Q = (0.1 * rs.randn(R.shape[1], d)).astype(np.float32)
    b0 = (0.01 * rs.randn(R.shape[1])).astype(np.float32)
    loss, lr = ("bpr", 0.2) if pairwise else ("square", 0.5)
    eng = FISMEngine(c1, Q, R, lr, [0.01, 0.02], 0.5, 33, bias=b0, learner="gd", loss=loss, pairwise=pairwise)
    st = F.State(c1, Q, b0, learner="gd", lr=lr)
    loss2 = torch.zeros(2, device=eng.c1.device)
    for k in range(2):
        fed, kept = _with_slots_that_take_no_part(R, rs, pairwise)
        got = _feed(eng, *fed, loss2)
        want = F.step(st, R, *kept, pairwise, loss, 0.5, [0.01, 0.02])
        print("step %d loss: device %.9g, restatement %.9g" % (k + 1, got, want))
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
        for name, t in zip(("c1", "Q", "bias"), _tables(eng)):
            err = np.abs(t - st.var[name]).max()
            print("step %d %s: err %.3g, bar %.3g" % (k + 1, name, err, 1e-5 * np.abs(st.var[name]).max()))
            assert err <= 1e-5 * np.abs(st.var[name]).max(), (name, k, err)


def test_embedding_size_129_is_refused():
    from neurec_amd.fism import FISMEngine
    R = _toy()
    z = np.zeros((R.shape[1], 129), np.float32)
    with pytest.raises(NotImplementedError, match="128"):
        FISMEngine(z, z, R, 0.01, [0.0, 0.0], 0.5, 8)


@pytest.mark.parametrize("case", ["square_adam", "bpr_adam"])
def test_two_engines_end_byte_identical(golden, case):
    import torch
    g = golden
    out = []
    for _ in range(2):
        eng = _engine(g, case)
        loss2 = torch.zeros(2, device=eng.c1.device)
        losses = [_feed(eng, g[case + "_users"][k], g[case + "_items"][k], g[case + "_third"][k], loss2)
                  for k in range(3)]
        out.append([t.clone() for t in (eng.c1, eng.Q, eng.bias)] + [losses])
    assert all(torch.equal(a, b) for a, b in zip(out[0][:3], out[1][:3])) and out[0][3] == out[1][3]


def test_device_stream_triples_follow_the_rule():
    """PointwiseSampler's device triples: label 1 <=> the item is in the user's train row (so the kernel's rule pools
    the history without it, n = |R_u|), label 0 <=> it is not (whole history, n = |R_u| + 1); nnz (1 + num_neg)
    instances an epoch.  It is here and not in test_fism_cpu.py because the sampler forms its epoch on the device;
    what carries weight is the label-in-row equivalence and the count (the (H, n) rule itself is pinned against the
    reference generator's own output in test_fism_cpu.py)"""
    from neurec_amd.data import PointwiseSampler
    R = _toy()

    class DS:
        num_users, num_items = R.shape

        def get_user_train_dict(self, by_time=False):
            return {u: R.indices[R.indptr[u]:R.indptr[u + 1]].tolist() for u in range(R.shape[0])
                    if R.indptr[u + 1] > R.indptr[u]}
    n = 0
    for users, items, labels in PointwiseSampler(DS(), neg_num=4, batch_size=256, shuffle=True, as_tensors=True):
        u, i, y = users.cpu().numpy(), items.cpu().numpy(), labels.cpu().numpy()
        inrow = np.asarray([R[a, b] != 0 for a, b in zip(u, i)])
        assert np.array_equal(inrow, y == 1.0)
        inst = F.instances(R, u, i, y, False)
        assert all(len(F.history(R, a, e)) + 1 == nn for a, _, e, nn, _ in inst)
        n += len(u)
    assert n == R.nnz * 5


# ------------------------------------------------------------------ drop-in
FISM_PROPERTIES = """[hyperparameters]
batch_size=256
epochs=100
embedding_size=16
regs=[1e-7,1e-7]
alpha=0.5
num_neg=4
learning_rate=0.01
learner=adam
topk=10
loss_function=square
is_pairwise=False
init_method=normal
stddev=0.01
verbose=1
"""


def _write_dataset(root, n_users=120, n_items=90, seed=3):
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "dataset"), exist_ok=True)
    with open(os.path.join(root, "dataset", "toy.rating"), "w") as f:
        for u in range(n_users):
            liked = (u % 6) * 15 + rng.choice(15, 10, replace=False)       # 6 taste clusters
            for it in liked:
                f.write("%d\t%d\t%d\t%d\n" % (u + 7, it + 300, 5, rng.randint(1, 10**6)))


def _run(tmp_path, argv):
    from neurec_amd.main import main
    path = defaults.write_default_configs(str(tmp_path), overrides={
        "data.input.path": os.path.join(str(tmp_path), "dataset"), "data.input.dataset": "toy",
        "test_batch_size": "64"})
    with open(os.path.join(str(tmp_path), "conf", "FISM.properties"), "w") as f:
        f.write(FISM_PROPERTIES)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return main(argv=argv, properties=path)
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("pairwise", [False, True])
def test_fism_config_drops_in(tmp_path, pairwise):
    from neurec_amd import engine as E
    import torch
    _write_dataset(str(tmp_path))
    argv = ["--recommender=FISM", "--epochs=2"] + (["--is_pairwise=True", "--loss_function=bpr"] if pairwise else [])
    model = _run(tmp_path, argv)
    folder = os.path.join(str(tmp_path), "log", "toy", "FISM")
    files = os.listdir(folder)
    assert len(files) == 1 and files[0].startswith("toy_FISM_")
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "FISM's hyperparameters:" in text
    assert ("pairwise structure: positive side = history without the item" in text) == pairwise
    assert ("pointwise structure:" in text) == (not pairwise)
    lines = [ln for ln in text.splitlines()
             if re.search(r"metrics:\t|\[iter \d+ : loss : [0-9.]+, time: [0-9.]+\]|epoch \d+:\t", ln)]
    kinds = [("m" if "metrics:" in ln else "i%s" % re.search(r"iter (\d+)", ln).group(1)
              if "[iter" in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)) for ln in lines]
    assert kinds == ["m", "i1", "e1", "i2", "e2"], kinds
    evals = re.findall(r"epoch (\d+):\t(.+)", text)
    # the logged metrics = an evaluation of predict()'s rows through eval_scores
    uni = model.evaluator.evaluator
    users = list(uni.user_pos_test.keys())
    st = uni._device(model.num_items)
    scores = torch.from_numpy(model.predict(users, None)).to(E.require_gpu())
    du = torch.tensor(np.asarray(users, dtype=np.int32), device=scores.device)
    E.mask_train(scores, du, st["train"])
    rows = E.eval_scores(scores, st["test"], uni.metrics, uni.max_top, users=du).cpu().numpy()
    assert uni._format(np.mean(rows, axis=0)).strip() == evals[-1][1].strip()
    full = model.predict([0, 5, 9], None)
    assert full.shape == (3, model.num_items) and full.dtype == np.float32
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])


def test_refusals(tmp_path, monkeypatch):
    _write_dataset(str(tmp_path))
    with pytest.raises(Exception, match="suitable loss function"):
        _run(tmp_path, ["--recommender=FISM", "--epochs=1", "--loss_function=hinge"])     # not a pointwise loss
    with pytest.raises(ValueError, match="suitable optimizer"):
        _run(tmp_path, ["--recommender=FISM", "--epochs=1", "--learner=lbfgs"])
    with pytest.raises(NotImplementedError):
        _run(tmp_path, ["--recommender=FISM", "--epochs=1", "--embedding_size=129"])
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)                                # WORLD_SIZE > 1
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(tmp_path, ["--recommender=FISM", "--epochs=1"])
