"""FPMC on the GPU (csrc/fpmc.hip through neurec_amd/fpmc.py): every step of the reference class's trace, predict(),
the edge shapes, long runs and the sort's second path against the float64 restatement, slots that take no part,
determinism, the refusals, the time-order samplers' contract and the drop-in run through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from neurec_amd import defaults
import fpmc_restatement as P
from fpmc_restatement import CASES

pytestmark = pytest.mark.gpu

SORT_ONE_WORKGROUP = 16384          # keys nrhip_sort_u64 sorts in one workgroup's LDS (csrc/bpr.hip: kPlanMaxKeys)


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_fpmc")


def _engine(g, case, **kw):
    from neurec_amd.fpmc import FPMCEngine
    loss, learner, pairwise = CASES[case]
    return FPMCEngine(g["UI_0"], g["IU_0"], g["IL_0"], g["LI_0"], float(g["learning_rate"]), float(g["reg_mf"]), 64,
                      loss=loss, pairwise=pairwise, learner=learner, **kw)


def _feed(eng, users, recent, items, third, loss2):
    import torch
    dev = eng.UI.device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    eng.step(t(users, torch.int32), t(recent, torch.int32), t(items, torch.int32),
             t(third, torch.int32 if eng.pairwise else torch.float32), loss2)
    return float(loss2.cpu().numpy().astype(np.float64).sum())


def _tables(eng):
    return [getattr(eng, k).cpu().numpy() for k in P.TABLES]


def _batch(g, case, k):
    return tuple(g["%s_%s" % (case, f)][k] for f in ("users", "recent", "items", "third"))


def _train(eng, g, case):
    import torch
    loss2 = torch.zeros(2, device=eng.UI.device)
    return [_feed(eng, *_batch(g, case, k), loss2) for k in range(len(g[case + "_users"]))]


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Tables and loss after every step against the f64 trace: within 4x the reference's own f32-to-f64 distance of
    that step and table (read from the golden) plus 1e-5 max|want|.  Rows outside <case>_rows_* are bit-equal to their
    initial value — under adam too: the sweep moves only rows whose m is non-zero, and those are rows that moved."""
    import torch
    g = golden
    eng = _engine(g, case)
    loss2 = torch.zeros(2, device=eng.UI.device)
    for k in range(len(g[case + "_users"])):
        loss = _feed(eng, *_batch(g, case, k), loss2)
        want, ref32 = g[case + "_f64_loss"][k], g[case + "_f32_loss"][k]
        print("%s step %d loss: device err %.3g, reference f32 err %.3g" % (case, k + 1, abs(loss - want),
                                                                           abs(ref32 - want)))
        assert abs(loss - want) <= 4 * abs(ref32 - want) + 1e-5 * abs(want)
        for name, got, w64, w32 in zip(P.TABLES, _tables(eng), P.golden_tables(g, case, "f64", k),
                                       P.golden_tables(g, case, "f32", k)):
            bar = np.abs(w32.astype(np.float64) - w64).max()
            err = np.abs(got.astype(np.float64) - w64).max()
            print("%s step %d %s: device err %.3g, reference f32 err %.3g" % (case, k + 1, name, err, bar))
            assert err <= 4 * bar + 1e-5 * np.abs(w64).max(), (case, k, name, err, bar)
            still = np.setdiff1d(np.arange(len(got)), g["%s_rows_%s" % (case, name)])
            assert len(still) and np.array_equal(got[still], g[name + "_0"][still]), (case, k, name)
    for name in P.TABLES:                                     # the gradient buffers are zero again
        assert not eng.G[name].any().item(), name


def test_predict_matches_the_reference(golden):
    """full and candidate mode after the trained case `ce_adam`; a user with no train items scores <UI_u, IU_i>"""
    g = golden
    users, cand = g["predict_users"], g["predict_cand"]
    seqs = P.sequences(g)
    last = P.last_items(seqs, int(g["shape"][0]))
    eng = _engine(g, "ce_adam")
    _train(eng, g, "ce_adam")
    w64, w32 = g["predict_f64"], g["predict_f32"]
    bound = 4 * np.abs(w32 - w64).max() + 1e-5 * np.abs(w64).max()
    got = eng.score(users, last).cpu().numpy().astype(np.float64)
    print("predict: device err %.3g, reference f32 err %.3g" % (np.abs(got - w64).max(), np.abs(w32 - w64).max()))
    assert got.shape == w64.shape and np.abs(got - w64).max() <= bound
    from neurec_amd.model.general_recommender._common import predict_scores
    Pf, Qf = eng.eval_factors(last)
    assert eng.eval_factors(last)[0] is Pf                   # rebuilt only after a step
    full = predict_scores(Pf, Qf, users.tolist(), None)
    assert np.abs(full - w64).max() <= bound
    got_c = predict_scores(Pf, Qf, users.tolist(), [c.tolist() for c in cand])
    c64, c32 = g["predict_cand_f64"], g["predict_cand_f32"]
    assert np.abs(np.stack(got_c) - c64).max() <= 4 * np.abs(c32 - c64).max() + 1e-5 * np.abs(c64).max()
    assert all(np.array_equal(r, full[k][c]) for k, (r, c) in enumerate(zip(got_c, cand)))
    empty = int(np.flatnonzero(last < 0)[0])
    UI, IU = eng.UI.cpu().numpy().astype(np.float64), eng.IU.cpu().numpy().astype(np.float64)
    want = IU @ UI[empty]
    got_e = eng.score(np.asarray([empty], np.int32), last).cpu().numpy()[0]
    assert np.abs(got_e - want).max() <= 1e-5 * np.abs(want).max()


def _tables0(U, I, d, seed, scale=0.1):
    rs = np.random.RandomState(seed)
    return [(scale * rs.randn(n, d)).astype(np.float32) for n in (U, I, I, I)]


def _random_batch(rs, U, I, B, pairwise):
    users = rs.randint(U, size=B).astype(np.int32)
    recent = rs.randint(I, size=B).astype(np.int32)
    items = rs.randint(I, size=B).astype(np.int32)
    third = rs.randint(I, size=B).astype(np.int32) if pairwise else (rs.rand(B) < 0.4).astype(np.float32)
    return users, recent, items, third


def _against_restatement(tabs, batches, pairwise, loss, lr, reg=0.01, learner="gd", max_batch=None):
    """the engine and the float64 restatement fed the same batches: loss and tables within 1e-5 max|want| after every
    step (fp32 storage of O(0.1) tables and fp32 loss sums).  The learner is plain gradient descent with a large step:
    the update is linear in the gradient, so a wrong or missing term of any gradient shows at its full size"""
    import torch
    from neurec_amd.fpmc import FPMCEngine
    eng = FPMCEngine(*tabs, lr, reg, max_batch or max(len(b[0]) for b in batches), loss=loss, pairwise=pairwise,
                     learner=learner)
    st = P.State(*tabs, learner=learner, lr=lr)
    loss2 = torch.zeros(2, device=eng.UI.device)
    for k, b in enumerate(batches):
        got = _feed(eng, *b, loss2)
        want = P.step(st, *b, pairwise, loss, reg)
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
        for name, t in zip(P.TABLES, _tables(eng)):
            err = np.abs(t - st.var[name]).max()
            assert err <= 1e-5 * np.abs(st.var[name]).max(), (name, k, err)
    return eng, st


@pytest.mark.parametrize("d", [1, 16, 20, 64, 128])
@pytest.mark.parametrize("mode,loss", [("pair", "bpr"), ("pair", "hinge"), ("pair", "square"),
                                       ("point", "cross_entropy"), ("point", "square")])
def test_edges_against_the_float64_restatement(d, mode, loss):
    """every lane layout (d = 1, 16, 20, 64, 128) crossed with batches of 1, 33, and 64 followed by a short last batch
    of 7, both modes and every loss of PAIRWISE_LOSSES / POINTWISE_LOSSES, two gd steps each: 23 users and 31 items,
    so every batch but the first holds rows many times over in every role"""
    pairwise = mode == "pair"
    U, I = 23, 31
    scale = 0.5 if d == 1 else 0.3 if d <= 20 else 0.1
    for sizes in ((1, 1), (33, 33), (64, 7)):
        rs = np.random.RandomState(1000 * d + sizes[0])
        batches = [_random_batch(rs, U, I, B, pairwise) for B in sizes]
        _against_restatement(_tables0(U, I, d, d, scale), batches, pairwise, loss, 0.2 if pairwise else 0.5)


@pytest.mark.parametrize("pairwise", [False, True])
def test_long_runs(pairwise):
    """U = 40, I = 50, d = 20, B = 128: one item is the target of 70 instances and the `recent` of 70 others, one user
    holds 70 instances — runs longer than a wavefront"""
    rs = np.random.RandomState(8)
    U, I, B = 40, 50, 128
    batches = []
    for _ in range(2):
        users, recent, items, third = _random_batch(rs, U, I, B, pairwise)
        order = rs.permutation(B)
        items[order[:70]] = 11
        recent[order[58:]] = 11
        users[rs.permutation(B)[:70]] = 3
        assert (items == 11).sum() >= 70 and (recent == 11).sum() >= 70 and (users == 3).sum() >= 70
        batches.append((users, recent, items, third))
    _against_restatement(_tables0(U, I, 20, 5), batches, pairwise, "bpr" if pairwise else "square", 0.02)


@pytest.mark.parametrize("pairwise", [False, True])
def test_one_batch_beyond_the_one_workgroup_sort(pairwise):
    """The step's one internal capacity is the sort of its 3 N keys: one workgroup's LDS network up to 16,384 keys,
    the segmented multi-workgroup network beyond.  The smallest batch whose keys exceed it (3 B or 6 B a multiple of 3:
    16,386 keys), against the restatement at d = 16; the largest batch below it takes the first path in every other
    test."""
    per = 6 if pairwise else 3
    B = SORT_ONE_WORKGROUP // per + 1
    assert per * (B - 1) <= SORT_ONE_WORKGROUP < per * B
    rs = np.random.RandomState(2)
    U, I = 900, 1100
    batches = [_random_batch(rs, U, I, B, pairwise)]
    _against_restatement(_tables0(U, I, 16, 6), batches, pairwise, "bpr" if pairwise else "square", 0.05)


@pytest.mark.parametrize("pairwise", [False, True])
def test_slots_that_take_no_part(pairwise):
    """a user id >= U (or negative) and an item, recent or negative outside [0, I): the slot takes no part — two gd
    steps give the loss and tables of the restatement fed the same batches without those slots (square / bpr: sums
    over the instances; the pointwise cross-entropy is a mean over the batch's length, those slots included)"""
    rs = np.random.RandomState(29)
    U, I, B = 23, 31, 33
    fed, kept = [], []
    for _ in range(2):
        users, recent, items, third = _random_batch(rs, U, I, B, pairwise)
        users[0], users[7], items[21], items[32], recent[12], recent[13] = -1, U, -1, I, I, -1
        out = [0, 7, 21, 32, 12, 13]
        if pairwise:
            third[5], third[30] = I, -1
            out += [5, 30]
        keep = np.setdiff1d(np.arange(B), out)
        fed.append((users, recent, items, third))
        kept.append(tuple(x[keep] for x in (users, recent, items, third)))
    import torch
    from neurec_amd.fpmc import FPMCEngine
    tabs = _tables0(U, I, 16, 3, 0.3)
    loss, lr = ("bpr", 0.2) if pairwise else ("square", 0.5)
    eng = FPMCEngine(*tabs, lr, 0.01, B, loss=loss, pairwise=pairwise, learner="gd")
    st = P.State(*tabs, learner="gd", lr=lr)
    loss2 = torch.zeros(2, device=eng.UI.device)
    for k in range(2):
        got = _feed(eng, *fed[k], loss2)
        want = P.step(st, *kept[k], pairwise, loss, 0.01)
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
        for name, t in zip(P.TABLES, _tables(eng)):
            err = np.abs(t - st.var[name]).max()
            assert err <= 1e-5 * np.abs(st.var[name]).max(), (name, k, err)


@pytest.mark.parametrize("case", ["square_adam", "bpr_adam", "square_momentum"])
def test_two_engines_end_byte_identical(golden, case):
    """the same three batches twice (the cases of two steps: the first batch again as the third)"""
    import torch
    g = golden
    out = []
    for _ in range(2):
        eng = _engine(g, case)
        loss2 = torch.zeros(2, device=eng.UI.device)
        n = len(g[case + "_users"])
        losses = [_feed(eng, *_batch(g, case, k % n), loss2) for k in range(3)]
        out.append([getattr(eng, k).clone() for k in P.TABLES] + [losses])
    assert all(torch.equal(a, b) for a, b in zip(out[0][:4], out[1][:4])) and out[0][4] == out[1][4]


def test_engine_refusals():
    import torch
    from neurec_amd.fpmc import FPMCEngine
    z = lambda n, d=4: np.zeros((n, d), np.float32)
    with pytest.raises(NotImplementedError, match="128"):
        FPMCEngine(z(5, 129), z(6, 129), z(6, 129), z(6, 129), 0.01, 0.0, 8)
    with pytest.raises(Exception, match="please choose a suitable loss function"):
        FPMCEngine(z(5), z(6), z(6), z(6), 0.01, 0.0, 8, loss="hinge", pairwise=False)
    with pytest.raises(Exception, match="please choose a suitable loss function"):
        FPMCEngine(z(5), z(6), z(6), z(6), 0.01, 0.0, 8, loss="cross_entropy", pairwise=True)
    with pytest.raises(ValueError, match="please select a suitable optimizer"):
        FPMCEngine(z(5), z(6), z(6), z(6), 0.01, 0.0, 8, learner="lbfgs")
    eng = FPMCEngine(z(5), z(6), z(6), z(6), 0.01, 0.0, 8, loss="square")
    i32 = torch.zeros(9, dtype=torch.int32, device=eng.UI.device)
    with pytest.raises(ValueError, match="max_batch"):
        eng.step(i32, i32, i32, torch.zeros(9, device=eng.UI.device), torch.zeros(2, device=eng.UI.device))


# ------------------------------------------------------------------ the samplers' contract
SEQS = {0: [3, 1, 4, 11, 5], 1: [9, 2], 2: [6], 3: [5, 3, 5 + 3, 0, 7, 10], 5: [2, 11, 1]}


class _ToyTimed:
    num_users, num_items = 6, 12

    def get_user_train_dict(self, by_time=False):
        return {u: (list(s) if by_time else sorted(s)) for u, s in SEQS.items()}


@pytest.mark.parametrize("pairwise", [False, True])
def test_time_order_samplers_feed_what_the_step_expects(pairwise):
    """one epoch of each time-order sampler at high_order = 1 with as_tensors=True on hand-written sequences: `recent`
    immediately precedes `item` (pairwise: the positive) in the user's by-time sequence, negatives and label-0 items
    lie outside the sequence, and every window comes once (pointwise: with num_neg label-0 instances)"""
    from neurec_amd.data import TimeOrderPairwiseSampler, TimeOrderPointwiseSampler
    n_windows = sum(len(s) - 1 for s in SEQS.values())
    if pairwise:
        it = TimeOrderPairwiseSampler(_ToyTimed(), high_order=1, neg_num=1, batch_size=4, shuffle=True, as_tensors=True)
    else:
        it = TimeOrderPointwiseSampler(_ToyTimed(), high_order=1, neg_num=2, batch_size=4, shuffle=True,
                                       as_tensors=True)
    seen, n = [], 0
    for users, recent, items, third in it:
        u, l, i, t = (x.cpu().numpy() for x in (users, recent, items, third))
        assert u.ndim == l.ndim == i.ndim == t.ndim == 1 and len(u) == len(l) == len(i) == len(t) <= 4
        for b in range(len(u)):
            s = SEQS[int(u[b])]
            if pairwise or t[b] == 1.0:
                k = s.index(int(i[b]))
                assert k > 0 and s[k - 1] == int(l[b])
                seen.append((int(u[b]), k))
                if pairwise:
                    assert int(t[b]) not in s and 0 <= int(t[b]) < 12
            else:
                assert t[b] == 0.0 and int(i[b]) not in s and int(l[b]) in s[:-1]
        n += len(u)
    assert sorted(seen) == sorted((u, k) for u, s in SEQS.items() for k in range(1, len(s)))
    assert n == (n_windows if pairwise else 3 * n_windows) and len(it) == -(-n // 4)


# ------------------------------------------------------------------ drop-in
FPMC_PROPERTIES = """[hyperparameters]
epochs=500
batch_size=512
embedding_size=16
reg_mf=0.01
learning_rate=0.001
learner=adam
is_pairwise=False
num_neg=4
loss_function=cross_entropy
init_method=uniform
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
        "test_batch_size": "64", "by_time": "True"})
    with open(os.path.join(str(tmp_path), "conf", "FPMC.properties"), "w") as f:
        f.write(FPMC_PROPERTIES)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return main(argv=argv, properties=path)
    finally:
        os.chdir(cwd)


def _host_metrics(scores, train, test, users, top_show, metric_ids):
    """the metrics `metric_ids` (metric.h:111-117: 1 Precision, 2 Recall, 3 MAP, 4 NDCG, 5 MRR), in that order, @
    top_show of `scores` rows on the host (metric.h:17-109), train items struck, the mean over the users"""
    K = int(max(top_show))
    rows = []
    for r, u in enumerate(users):
        s = scores[r].astype(np.float64).copy()
        s[train.get(u, [])] = -np.inf
        top = np.argsort(-s, kind="stable")[:K]
        truth = set(test[u])
        hit = np.asarray([int(i) in truth for i in top], np.float64)
        ranks = np.arange(1, K + 1)
        hits = np.cumsum(hit)
        prec, rec = hits / ranks, hits / len(truth)
        ap = np.cumsum(hit * prec) / np.minimum(len(truth), ranks)
        disc = 1.0 / np.log2(ranks + 1)
        ndcg = np.cumsum(hit * disc) / np.cumsum(disc * (ranks <= len(truth)))
        first = np.flatnonzero(hit)
        mrr = np.where(ranks > first[0], 1.0 / (first[0] + 1), 0.0) if len(first) else np.zeros(K)
        by_id = {1: prec, 2: rec, 3: ap, 4: ndcg, 5: mrr}
        rows.append(np.stack([by_id[m] for m in metric_ids]))
    mean = np.mean(rows, axis=0)
    return mean[:, np.asarray(top_show) - 1].reshape(-1)


@pytest.mark.parametrize("pairwise", [False, True])
def test_fpmc_config_drops_in(tmp_path, monkeypatch, pairwise):
    """NeuRec.properties + the reference's conf/FPMC.properties + a UIRT file with by_time=True: two epochs through
    neurec_amd.main in both modes; the reference's log lines and the deviation line; the epoch-1 loss against the
    restatement on the same stream; the evaluation through the factor path, its metrics against the host's"""
    from neurec_amd.data import TimeOrderPairwiseSampler, TimeOrderPointwiseSampler
    from neurec_amd.util.tool import get_initializer
    _write_dataset(str(tmp_path))
    argv = ["--recommender=FPMC", "--epochs=2"] + (["--is_pairwise=True", "--loss_function=bpr"] if pairwise else [])
    model = _run(tmp_path, argv)
    folder = os.path.join(str(tmp_path), "log", "toy", "FPMC")
    files = os.listdir(folder)
    assert len(files) == 1 and files[0].startswith("toy_FPMC_")
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "FPMC's hyperparameters:" in text
    assert "users without train items score <UI_u, IU_i> alone (the reference raises KeyError)" in text
    lines = [ln for ln in text.splitlines()
             if re.search(r"metrics:\t|\[iter \d+ : loss : [0-9.]+, time: [0-9.]+\]|epoch \d+:\t", ln)]
    kinds = [("m" if "metrics:" in ln else "i%s" % re.search(r"iter (\d+)", ln).group(1)
              if "[iter" in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)) for ln in lines]
    assert kinds == ["m", "i1", "e1", "i2", "e2"], kinds                  # no evaluation before the first epoch
    evals = re.findall(r"epoch (\d+):\t(.+)", text)
    shown = np.asarray([float(x) for x in evals[-1][1].split()])
    assert np.all(np.isfinite(shown)) and shown.max() > 0

    # the epoch-1 loss: the same stream (the sampler's epoch 0) through the restatement, over the number of BATCHES
    ds = model.dataset
    if pairwise:
        it = TimeOrderPairwiseSampler(ds, high_order=1, neg_num=1, batch_size=512, shuffle=True, as_tensors=True)
    else:
        it = TimeOrderPointwiseSampler(ds, high_order=1, neg_num=4, batch_size=512, shuffle=True, as_tensors=True)
    init = get_initializer("uniform", 0.01, seed=2017)
    d = 16
    tabs = [init([n, d]) for n in (ds.num_users, ds.num_items, ds.num_items, ds.num_items)]
    st = P.State(*tabs, learner="adam", lr=0.001)
    total = 0.0
    for batch in it:
        total += P.step(st, *[x.cpu().numpy() for x in batch], pairwise, "bpr" if pairwise else "cross_entropy", 0.01)
    logged = float(re.search(r"\[iter 1 : loss : ([0-9.]+),", text).group(1))
    want = total / len(it)
    print("epoch-1 loss: logged %.6f, restatement %.9f" % (logged, want))
    assert abs(logged - want) <= 1e-4 * abs(want)

    # the evaluator took the factor path (predict is never called), and its metrics are the host's on engine.score
    uni = model.evaluator.evaluator
    monkeypatch.setattr(model, "predict", lambda *a, **k: (_ for _ in ()).throw(AssertionError("predict called")))
    again = np.asarray([float(x) for x in model.evaluator.evaluate(model).split()])
    assert np.array_equal(again, shown)
    monkeypatch.undo()
    users = list(uni.user_pos_test.keys())
    scores = model.engine.score(np.asarray(users, np.int32), model.last_items).cpu().numpy()
    host = _host_metrics(scores, uni.user_pos_train, uni.user_pos_test, users, uni.top_show, uni.metrics)
    print("metrics: evaluator %s\n         host      %s" % (shown, host))
    assert np.abs(host - shown).max() <= 1e-6
    full = model.predict([0, 5, 9], None)
    assert full.shape == (3, model.num_items) and full.dtype == np.float32
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])


def test_refusals(tmp_path, monkeypatch):
    _write_dataset(str(tmp_path))
    with pytest.raises(Exception, match="suitable loss function"):
        _run(tmp_path, ["--recommender=FPMC", "--epochs=1", "--loss_function=hinge"])     # not a pointwise loss
    with pytest.raises(ValueError, match="suitable optimizer"):
        _run(tmp_path, ["--recommender=FPMC", "--epochs=1", "--learner=lbfgs"])
    with pytest.raises(NotImplementedError, match="128"):
        _run(tmp_path, ["--recommender=FPMC", "--epochs=1", "--embedding_size=129"])
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)                                # WORLD_SIZE > 1
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(tmp_path, ["--recommender=FPMC", "--epochs=1"])
