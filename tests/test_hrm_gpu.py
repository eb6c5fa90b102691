"""HRM on the GPU (csrc/hrm.hip through neurec_amd/hrm.py): every step of the reference class's trace, predict(), the
edge shapes, constructed ties, long runs and the sort's second path against the float64 restatement, slots that take no
part, determinism, the refusals, the time-order sampler's contract and the drop-in run through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from neurec_amd import defaults
import hrm_restatement as P
from hrm_restatement import CASES

pytestmark = pytest.mark.gpu

SORT_ONE_WORKGROUP = 16384          # keys nrhip_sort_u64 sorts in one workgroup's LDS (csrc/bpr.hip: kPlanMaxKeys)
PAIRS = [("max", "max"), ("max", "avg"), ("avg", "max"), ("avg", "avg")]


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_hrm")


def _engine(g, case, **kw):
    from neurec_amd.hrm import HRMEngine
    loss, learner, pre, ses, L = CASES[case]
    return HRMEngine(g["P_0"], g["V_0"], float(g["learning_rate"]), float(g["reg_mf"]), 64, L, pre_agg=pre,
                     session_agg=ses, loss=loss, learner=learner, **kw)


def _feed(eng, users, recents, items, labels, loss2):
    import torch
    dev = eng.P.device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    eng.step(t(users, torch.int32), t(recents, torch.int32), t(items, torch.int32), t(labels, torch.float32), loss2)
    return float(loss2.cpu().numpy().astype(np.float64).sum())


def _tables(eng):
    return [getattr(eng, k).cpu().numpy() for k in P.TABLES]


def _batch(g, case, k):
    return tuple(g["%s_%s" % (case, f)][k] for f in ("users", "recents", "items", "labels"))


def _train(eng, g, case):
    import torch
    loss2 = torch.zeros(2, device=eng.P.device)
    return [_feed(eng, *_batch(g, case, k), loss2) for k in range(len(g[case + "_users"]))]


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Tables and loss after every step against the f64 trace: within 4x the reference's own f32-to-f64 distance of
    that step and table (read from the golden) plus 1e-5 max|want|.  Every max case holds, in every step, a session
    tie and a user-vs-session tie (test_hrm_cpu.py).  Rows outside <case>_rows_* are bit-equal to their initial value;
    the gradient buffers are zero afterwards."""
    import torch
    g = golden
    eng = _engine(g, case)
    loss2 = torch.zeros(2, device=eng.P.device)
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
    """full and candidate mode after the trained case `ce_adam_max_max` (users with |R_u| >= L, = 2 and = 1 among
    them); eval_factors is rebuilt only after a step; the empty user (deviation a), every user with |R_u| < L and an
    L = 1 engine (deviation b) against the restatement"""
    import torch
    from neurec_amd.model.general_recommender._common import predict_scores
    from neurec_amd.model.sequential_recommender.HRM import last_items_table
    g = golden
    case = P.PREDICT_CASE
    _, _, pre, ses, L = CASES[case]
    users, cand = g["predict_users"], g["predict_cand"]
    seqs = P.sequences(g)
    U = int(g["shape"][0])
    last = last_items_table(seqs, U, L)
    eng = _engine(g, case, last_items=last)
    _train(eng, g, case)
    w64, w32 = g["predict_f64"], g["predict_f32"]
    bound = 4 * np.abs(w32 - w64).max() + 1e-5 * np.abs(w64).max()
    got = eng.score(users).cpu().numpy().astype(np.float64)
    print("predict: device err %.3g, reference f32 err %.3g" % (np.abs(got - w64).max(), np.abs(w32 - w64).max()))
    assert got.shape == w64.shape and np.abs(got - w64).max() <= bound
    Pf, Qf = eng.eval_factors()
    assert eng.eval_factors()[0] is Pf                       # rebuilt only after a step
    full = predict_scores(Pf, Qf, users.tolist(), None)
    assert np.abs(full - w64).max() <= bound
    got_c = predict_scores(Pf, Qf, users.tolist(), [c.tolist() for c in cand])
    c64, c32 = g["predict_cand_f64"], g["predict_cand_f32"]
    assert np.abs(np.stack(got_c) - c64).max() <= 4 * np.abs(c32 - c64).max() + 1e-5 * np.abs(c64).max()
    assert all(np.array_equal(r, full[k][c]) for k, (r, c) in enumerate(zip(got_c, cand)))
    # the empty user and every user with fewer than L items, against the restatement on the engine's own tables
    Pt, Vt = _tables(eng)
    short = np.asarray([u for u in range(U) if len(seqs.get(u, [])) < L], np.int32)
    assert any(u not in seqs for u in short.tolist()) and {len(seqs.get(u, [])) for u in short.tolist()} >= {0, 1, 2}
    want = P.predict(Pt, Vt, short, last, pre, ses)
    got_s = eng.score(short).cpu().numpy()
    assert np.abs(got_s - want).max() <= 1e-5 * np.abs(want).max()
    empty = int([u for u in short.tolist() if u not in seqs][0])
    k = short.tolist().index(empty)
    assert np.abs(got_s[k] - Vt.astype(np.float64) @ Pt[empty].astype(np.float64)).max() <= 1e-5 * np.abs(want).max()
    _feed(eng, *_batch(g, case, 0), torch.zeros(2, device=eng.P.device))
    assert eng.eval_factors()[0] is not Pf
    # L = 1: the user pooled with its last item, under both pre_aggs
    for one in ("one_max", "one_avg"):
        e1 = _engine(g, one, last_items=last_items_table(seqs, U, 1))
        _train(e1, g, one)
        every = np.arange(U, dtype=np.int32)
        want = P.predict(*_tables(e1), every, P.last_items_table(seqs, U, 1), CASES[one][2], CASES[one][3])
        assert np.abs(e1.score(every).cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()


def _tables0(U, I, d, seed, scale=0.1):
    rs = np.random.RandomState(seed)
    return [(scale * rs.randn(n, d)).astype(np.float32) for n in (U, I)]


def _random_batch(rs, U, I, B, L):
    users = rs.randint(U, size=B).astype(np.int32)
    recents = rs.randint(I, size=(B, L)).astype(np.int32)
    items = rs.randint(I, size=B).astype(np.int32)
    return users, recents, items, (rs.rand(B) < 0.4).astype(np.float32)


def _against_restatement(tabs, batches, L, pre, ses, loss, lr, reg=0.01, learner="gd", max_batch=None):
    """the engine and the float64 restatement fed the same batches: loss and tables within 1e-5 max|want| after every
    step (fp32 storage of O(0.1) tables and fp32 loss sums; FPMC's bound).  The learner is plain gradient descent with
    a large step: the update is linear in the gradient, so a wrong or missing term of any gradient — a share sent to
    the wrong row — shows at its full size"""
    import torch
    from neurec_amd.hrm import HRMEngine
    eng = HRMEngine(*tabs, lr, reg, max_batch or max(len(b[0]) for b in batches), L, pre_agg=pre, session_agg=ses,
                    loss=loss, learner=learner)
    st = P.State(*tabs, learner=learner, lr=lr)
    loss2 = torch.zeros(2, device=eng.P.device)
    for k, b in enumerate(batches):
        got = _feed(eng, *b, loss2)
        want = P.step(st, *b, loss, reg, pre, ses)
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
        for name, t in zip(P.TABLES, _tables(eng)):
            err = np.abs(t - st.var[name]).max()
            assert err <= 1e-5 * np.abs(st.var[name]).max(), (name, k, err)
    return eng, st


# every d at L = 16 max/max, every L at d = 20, the four aggregation pairs at (20, 3) and (16, 2), and the widest and
# the narrowest layout under avg
EDGES = [(d, 16, "max", "max") for d in (1, 16, 20, 64, 128)] + [(20, L, "max", "max") for L in (1, 2, 3)] + \
        [(20, 3, p, s) for p, s in PAIRS[1:]] + [(16, 2, p, s) for p, s in PAIRS[1:]] + \
        [(128, 3, "avg", "avg"), (64, 2, "max", "avg"), (1, 1, "avg", "max"), (1, 2, "avg", "max")]


@pytest.mark.parametrize("loss", ["cross_entropy", "square"])
@pytest.mark.parametrize("d,L,pre,ses", EDGES)
def test_edges_against_the_float64_restatement(d, L, pre, ses, loss):
    """every lane layout (d = 1, 16, 20, 64, 128), L = 1, 2, 3, 16, the four aggregation pairs and both losses, with
    batches of 1, 33, and 64 followed by a short last batch of 7, two gd steps each: 23 users and 31 items, the recents
    drawn with randint, so at L = 16 most instances hold an item twice (the self-tie) and every batch but the first
    holds rows many times over in every role"""
    U, I = 23, 31
    scale = 0.5 if d == 1 else 0.3 if d <= 20 else 0.1
    twice = 0
    for sizes in ((1, 1), (33, 33), (64, 7)):
        rs = np.random.RandomState(1000 * d + 10 * L + sizes[0])
        batches = [_random_batch(rs, U, I, B, L) for B in sizes]
        twice += sum(len(set(r)) < L for b in batches for r in b[1].tolist())
        _against_restatement(_tables0(U, I, d, d, scale), batches, L, pre, ses, loss, 0.5)
    assert L < 16 or twice > 100


def test_constructed_ties_split_exactly():
    """Two instances on dyadic tables, square loss, reg = 0, one gd step at lr = 1/4: P[u] equals the session row in a
    column (half to each), two recents share a column's max (half each), three share another (a third each: the
    derivative there is 21/16, a multiple of three), one item stands twice among an instance's recents and ties with
    itself, and V[0] is a recent here and the target there.  Every share, product and update is exact in fp32: the
    restatement run in float32 equals the float64 one exactly (checked first), and the device equals both bit for
    bit."""
    V = np.array([[0.5, 0.5, 0.25, 0.5], [0.5, 0.5, 0.25, 0.25], [0.25, 0.5, 1.0, 0.125], [0.125, 0.25, 0.5, 0.125],
                  [1.0, 1.0, 1.0, 1.0], [1.0, 0.75, 0.5, 0.25]], np.float32)
    Pt = np.array([[0.25, 0.125, 1.0, 2.0], [0.5, 0.25, 0.125, 0.0625], [3.0, 3.0, 3.0, 3.0]], np.float32)
    users, recents = np.array([0, 1], np.int32), np.array([[0, 1, 2], [1, 1, 3]], np.int32)
    items, labels = np.array([5, 0], np.int32), np.array([1.0, 0.0], np.float32)
    lr = 0.25
    out = {}
    for dt in (np.float32, np.float64):
        loss, GP, GV = P.gradients(Pt.astype(dt), V.astype(dt), users, recents, items, labels, "square", 0.0, "max",
                                   "max")
        out[dt] = (loss, Pt.astype(dt) - dt(lr) * GP, V.astype(dt) - dt(lr) * GV, GP, GV)
    l64, P64, V64, GP, GV = out[np.float64]
    assert out[np.float32][0] == l64 == 1.328125
    assert np.array_equal(out[np.float32][1].astype(np.float64), P64) and np.array_equal(P64.astype(np.float32), P64)
    assert np.array_equal(out[np.float32][2].astype(np.float64), V64) and np.array_equal(V64.astype(np.float32), V64)
    # the shares themselves: g = 1.75 and 1.5
    assert GV[0].tolist() == [0.875 + 0.75, 0.4375 + 0.75, 0.75, 0.375]        # a recent there, the target here
    assert GV[5].tolist() == [0.875, 0.875, 1.75, 3.5]
    assert GV[1].tolist() == [0.875 + 0.375, 0.4375 + 0.75, 0.0, 0.75] and GV[2].tolist() == [0.0, 0.4375, 0.4375, 0.0]
    assert GV[3].tolist() == [0.0, 0.0, 0.375, 0.0] and not GV[4].any()
    assert GP.tolist() == [[0.0, 0.0, 0.4375, 0.4375], [0.375, 0.0, 0.0, 0.0], [0.0] * 4]
    import torch
    from neurec_amd.hrm import HRMEngine
    eng = HRMEngine(Pt, V, lr, 0.0, 2, 3, pre_agg="max", session_agg="max", loss="square", learner="gd")
    loss2 = torch.zeros(2, device=eng.P.device)
    got = _feed(eng, users, recents, items, labels, loss2)
    assert got == l64 and loss2.cpu().numpy().tolist() == [1.328125, 0.0]
    assert np.array_equal(eng.P.cpu().numpy(), P64.astype(np.float32))
    assert np.array_equal(eng.V.cpu().numpy(), V64.astype(np.float32))


def test_long_runs():
    """U = 40, I = 50, d = 20, B = 128, L = 3: one item is the target of 70 instances and stands among the recents of
    more than 70 others (twice in many), one user holds 70 instances — runs longer than a wavefront"""
    rs = np.random.RandomState(8)
    U, I, B, L = 40, 50, 128, 3
    batches = []
    for _ in range(2):
        users, recents, items, labels = _random_batch(rs, U, I, B, L)
        order = rs.permutation(B)
        items[order[:70]] = 11
        recents[order[50:], rs.randint(L, size=B - 50)] = 11
        recents[order[100:], 0] = 11
        users[rs.permutation(B)[:70]] = 3
        assert (items == 11).sum() >= 70 and (recents == 11).any(axis=1).sum() >= 70 and (users == 3).sum() >= 70
        batches.append((users, recents, items, labels))
    _against_restatement(_tables0(U, I, 20, 5), batches, L, "max", "max", "square", 0.02)


def test_one_batch_beyond_the_one_workgroup_sort():
    """The step's one internal capacity is the sort of its B (L + 2) keys: one workgroup's LDS network up to 16,384
    keys, the segmented multi-workgroup network beyond.  The smallest batch whose keys exceed it at L = 2 (4,097 slots:
    16,388 keys), against the restatement at d = 16; every other test takes the first path."""
    L = 2
    B = SORT_ONE_WORKGROUP // (L + 2) + 1
    assert (L + 2) * (B - 1) <= SORT_ONE_WORKGROUP < (L + 2) * B
    rs = np.random.RandomState(2)
    U, I = 900, 1100
    _against_restatement(_tables0(U, I, 16, 6), [_random_batch(rs, U, I, B, L)], L, "max", "max", "square", 0.05)


def test_slots_that_take_no_part():
    """a user id >= U (or negative) and an item or any one recent outside [0, I): the slot takes no part — two gd steps
    give the loss and tables of the restatement fed the same batches without those slots (square: a sum over the
    instances)"""
    import torch
    from neurec_amd.hrm import HRMEngine
    rs = np.random.RandomState(29)
    U, I, B, L = 23, 31, 33, 3
    fed, kept = [], []
    for _ in range(2):
        users, recents, items, labels = _random_batch(rs, U, I, B, L)
        users[0], users[7], items[21], items[32], recents[12, 0], recents[13, 2], recents[14, 1] = -1, U, -1, I, I, -1, I
        keep = np.setdiff1d(np.arange(B), [0, 7, 21, 32, 12, 13, 14])
        fed.append((users, recents, items, labels))
        kept.append(tuple(x[keep] for x in (users, recents, items, labels)))
    tabs = _tables0(U, I, 16, 3, 0.3)
    eng = HRMEngine(*tabs, 0.5, 0.01, B, L, loss="square", learner="gd")
    st = P.State(*tabs, learner="gd", lr=0.5)
    loss2 = torch.zeros(2, device=eng.P.device)
    for k in range(2):
        got = _feed(eng, *fed[k], loss2)
        want = P.step(st, *kept[k], "square", 0.01, "max", "max")
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
        for name, t in zip(P.TABLES, _tables(eng)):
            err = np.abs(t - st.var[name]).max()
            assert err <= 1e-5 * np.abs(st.var[name]).max(), (name, k, err)


@pytest.mark.parametrize("case", ["square_adam", "square_momentum"])
def test_two_engines_end_byte_identical(golden, case):
    """the same three batches twice under max/max (the cases of two steps: the first batch again as the third)"""
    import torch
    g = golden
    out = []
    for _ in range(2):
        eng = _engine(g, case)
        loss2 = torch.zeros(2, device=eng.P.device)
        n = len(g[case + "_users"])
        losses = [_feed(eng, *_batch(g, case, k % n), loss2) for k in range(3)]
        out.append([getattr(eng, k).clone() for k in P.TABLES] + [losses])
    assert all(torch.equal(a, b) for a, b in zip(out[0][:2], out[1][:2])) and out[0][2] == out[1][2]


def test_engine_refusals():
    import torch
    from neurec_amd.hrm import HRMEngine
    z = lambda n, d=4: np.zeros((n, d), np.float32)
    with pytest.raises(NotImplementedError, match="128"):
        HRMEngine(z(5, 129), z(6, 129), 0.01, 0.0, 8, 2)
    with pytest.raises(NotImplementedError, match="embedding_size=0"):
        HRMEngine(z(5, 0), z(6, 0), 0.01, 0.0, 8, 2)
    with pytest.raises(NotImplementedError, match="high_order=0 is not supported \\(1 to 16\\)"):
        HRMEngine(z(5), z(6), 0.01, 0.0, 8, 0)
    with pytest.raises(NotImplementedError, match="high_order=17 is not supported \\(1 to 16\\)"):
        HRMEngine(z(5), z(6), 0.01, 0.0, 8, 17)
    with pytest.raises(Exception, match="please choose a suitable loss function"):
        HRMEngine(z(5), z(6), 0.01, 0.0, 8, 2, loss="bpr")
    with pytest.raises(ValueError, match="please select a suitable optimizer"):
        HRMEngine(z(5), z(6), 0.01, 0.0, 8, 2, learner="lbfgs")
    eng = HRMEngine(z(5), z(6), 0.01, 0.0, 8, 2, loss="square")
    dev = eng.P.device
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    loss2 = torch.zeros(2, device=dev)
    with pytest.raises(ValueError, match="max_batch"):
        eng.step(i32(9), i32(18), i32(9), torch.zeros(9, device=dev), loss2)
    with pytest.raises(ValueError, match="high_order = 2 entries per slot"):
        eng.step(i32(4), i32(4), i32(4), torch.zeros(4, device=dev), loss2)
    with pytest.raises(ValueError, match="same length"):
        eng.step(i32(4), i32(8), i32(3), torch.zeros(4, device=dev), loss2)
    with pytest.raises(ValueError, match="same length"):
        eng.step(i32(4), i32(8), i32(4), torch.zeros(5, device=dev), loss2)
    with pytest.raises(ValueError, match="last items"):
        eng.score(np.arange(2, dtype=np.int32))
    assert eng.t == 0 and not eng.G["V"].any().item()


# ------------------------------------------------------------------ the sampler's contract
SEQS = {0: [3, 1, 4, 11, 5, 9], 1: [9, 2], 2: [6], 3: [5, 3, 8, 0, 7, 10, 2], 5: [2, 11, 1, 4]}


class _ToyTimed:
    num_users, num_items = 6, 12

    def get_user_train_dict(self, by_time=False):
        return {u: (list(s) if by_time else sorted(s)) for u, s in SEQS.items()}


@pytest.mark.parametrize("L", [1, 3])
def test_time_order_sampler_feeds_what_the_step_expects(L):
    """one epoch of TimeOrderPointwiseSampler at high_order = L with as_tensors=True on hand-written sequences: the
    `recent` field reshaped to [B, L], as the plugin feeds it, holds the L items before `item` in the user's sequence;
    label-0 slots carry a window's recents and an item outside the sequence; every window comes once; and the engine
    takes the batches as they come"""
    import torch
    from neurec_amd.data import TimeOrderPointwiseSampler
    from neurec_amd.hrm import HRMEngine
    it = TimeOrderPointwiseSampler(_ToyTimed(), high_order=L, neg_num=2, batch_size=4, shuffle=True, as_tensors=True)
    tabs = _tables0(6, 12, 8, 1)
    eng = HRMEngine(*tabs, 0.1, 0.0, 4, L, loss="square", learner="gd")
    st = P.State(*tabs, learner="gd", lr=0.1)
    loss2 = torch.zeros(2, device=eng.P.device)
    seen, n = [], 0
    for users, recent, items, labels in it:
        rec = recent.reshape(-1, L)
        assert rec.is_contiguous() and tuple(rec.shape) == (users.numel(), L) and users.numel() <= 4
        u, r, i, t = (x.cpu().numpy() for x in (users, rec, items, labels))
        for b in range(len(u)):
            s = SEQS[int(u[b])]
            if t[b] == 1.0:
                k = s.index(int(i[b]))
                assert k >= L and r[b].tolist() == s[k - L:k]
                seen.append((int(u[b]), k))
            else:
                assert t[b] == 0.0 and int(i[b]) not in s
                assert any(r[b].tolist() == s[k - L:k] for k in range(L, len(s)))
        n += len(u)
        eng.step(users, rec, items, labels, loss2)
        want = P.step(st, u, r, i, t, "square", 0.0, "max", "max")
        # the square loss of a short batch can lie near zero, where a relative bound says nothing: per instance x is a
        # sum of d = 8 fp32 products of entries below 0.5 (error <= 9 * 2^-24 * 8 * 0.25 = 1.1e-6), and (y - x)^2 moves
        # by 2 |y - x| <= 2.5 times that
        assert abs(float(loss2.sum()) - want) <= 1e-5 * abs(want) + 3e-6 * len(u)
    n_windows = sum(max(len(s) - L, 0) for s in SEQS.values())
    assert sorted(seen) == sorted((u, k) for u, s in SEQS.items() for k in range(L, len(s)))
    assert n == 3 * n_windows and len(it) == -(-n // 4)
    for name, t in zip(P.TABLES, _tables(eng)):
        assert np.abs(t - st.var[name]).max() <= 1e-5 * np.abs(st.var[name]).max()


# ------------------------------------------------------------------ drop-in
HRM_PROPERTIES = """[hyperparameters]
epochs=3
batch_size=256
embedding_size=16
reg_mf=0
topK=10
learning_rate=0.001
learner=adam
#max,avg
pre_agg=max
#max,avg
session_agg=max
high_order=2

num_neg=4
#cross_entropy,square
loss_function=cross_entropy
init_method=normal
stddev=0.01
verbose=1
"""


def _run(tmp_path, argv):
    from neurec_amd.main import main
    path = defaults.write_default_configs(str(tmp_path), overrides={
        "data.input.path": os.path.join(str(tmp_path), "dataset"), "data.input.dataset": "toy",
        "test_batch_size": "64", "by_time": "True"})
    with open(os.path.join(str(tmp_path), "conf", "HRM.properties"), "w") as f:
        f.write(HRM_PROPERTIES)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return main(argv=argv, properties=path)
    finally:
        os.chdir(cwd)


def test_hrm_config_drops_in(tmp_path, monkeypatch):
    """NeuRec.properties + the reference's conf/HRM.properties + a UIRT file with by_time=True: two epochs through
    neurec_amd.main; the reference's log lines and the deviation line; the epoch-1 loss against the restatement on the
    same stream, over the number of BATCHES; the evaluation through the factor path, its metrics against the host's on
    predict() (1e-6, the bound test_fpmc_config_drops_in holds)"""
    from test_fpmc_gpu import _host_metrics, _write_dataset
    from neurec_amd.data import TimeOrderPointwiseSampler
    from neurec_amd.model.sequential_recommender.HRM import DEVIATIONS
    from neurec_amd.util.tool import get_initializer
    _write_dataset(str(tmp_path))
    model = _run(tmp_path, ["--recommender=HRM", "--epochs=2"])
    folder = os.path.join(str(tmp_path), "log", "toy", "HRM")
    files = os.listdir(folder)
    assert len(files) == 1 and files[0].startswith("toy_HRM_")
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "HRM's hyperparameters:" in text and DEVIATIONS in text
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
    it = TimeOrderPointwiseSampler(ds, high_order=2, neg_num=4, batch_size=256, shuffle=True, as_tensors=True)
    init = get_initializer("normal", 0.01, seed=2017)
    st = P.State(init([ds.num_users, 16]), init([ds.num_items, 16]), learner="adam", lr=0.001)
    total = 0.0
    for users, recent, items, labels in it:
        total += P.step(st, users.cpu().numpy(), recent.reshape(-1, 2).cpu().numpy(), items.cpu().numpy(),
                        labels.cpu().numpy(), "cross_entropy", 0.0, "max", "max")
    logged = float(re.search(r"\[iter 1 : loss : ([0-9.]+),", text).group(1))
    want = total / len(it)
    print("epoch-1 loss: logged %.6f, restatement %.9f" % (logged, want))
    assert abs(logged - want) <= 1e-4 * abs(want)

    # the evaluator took the factor path (predict is never called), and its metrics are the host's on predict()
    uni = model.evaluator.evaluator
    monkeypatch.setattr(model, "predict", lambda *a, **k: (_ for _ in ()).throw(AssertionError("predict called")))
    again = np.asarray([float(x) for x in model.evaluator.evaluate(model).split()])
    assert np.array_equal(again, shown)
    monkeypatch.undo()
    users = list(uni.user_pos_test.keys())
    scores = model.predict(users, None)
    assert scores.shape == (len(users), model.num_items) and scores.dtype == np.float32
    host = _host_metrics(scores, uni.user_pos_train, uni.user_pos_test, users, uni.top_show, uni.metrics)
    print("metrics: evaluator %s\n         host      %s" % (shown, host))
    assert np.abs(host - shown).max() <= 1e-6
    full = model.predict([0, 5, 9], None)
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])


def test_refusals(tmp_path, monkeypatch):
    from test_fpmc_gpu import _write_dataset
    _write_dataset(str(tmp_path))
    with pytest.raises(Exception, match="suitable loss function"):
        _run(tmp_path, ["--recommender=HRM", "--epochs=1", "--loss_function=bpr"])        # not a pointwise loss
    with pytest.raises(ValueError, match="suitable optimizer"):
        _run(tmp_path, ["--recommender=HRM", "--epochs=1", "--learner=lbfgs"])
    with pytest.raises(NotImplementedError, match="128"):
        _run(tmp_path, ["--recommender=HRM", "--epochs=1", "--embedding_size=129"])
    with pytest.raises(NotImplementedError, match="1 to 16"):
        _run(tmp_path, ["--recommender=HRM", "--epochs=1", "--high_order=17"])
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)                                # WORLD_SIZE > 1
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(tmp_path, ["--recommender=HRM", "--epochs=1"])
