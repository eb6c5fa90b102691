"""NPE on the GPU (csrc/npe.hip through neurec_amd/npe.py): every step of the reference class's trace, predict(), the
edge shapes, a constructed exact case of the gates, long runs and the sort's second path against the float64
restatement, slots that take no part, determinism, the refusals and the drop-in run through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from neurec_amd import defaults
import npe_restatement as P
from npe_restatement import CASES

pytestmark = pytest.mark.gpu

SORT_ONE_WORKGROUP = 16384          # keys nrhip_sort_u64 sorts in one workgroup's LDS (csrc/bpr.hip: kPlanMaxKeys)


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_npe")


def _engine(g, case, **kw):
    from neurec_amd.npe import NPEEngine
    loss, learner, L = CASES[case]
    return NPEEngine(g["P_0"], g["V_0"], g["W_0"], float(g["learning_rate"]), float(g["reg"]), 64, L, loss=loss,
                     learner=learner, **kw)


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
    that step and table (read from the golden) plus 1e-5 max|want|.  Every step holds a column with P[u] = 0, one with
    V[i] = 0 and one with a cancelled context sum (test_npe_cpu.py).  Rows outside <case>_rows_* are bit-equal to
    their initial value; the gradient buffers are zero afterwards."""
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
    """full and candidate mode after the trained case `ce_adam` (users with |R_u| >= L, = 2 and = 1 among them);
    eval_factors is rebuilt only after a step and its item side is relu(V) bit for bit; the empty user (deviation a),
    every user with |R_u| < L and an L = 1 engine (deviation b) against the restatement"""
    import torch
    from neurec_amd.model.general_recommender._common import predict_scores
    from neurec_amd.model.sequential_recommender.HRM import last_items_table
    from neurec_amd.npe import NPEEngine
    g = golden
    case = P.PREDICT_CASE
    L = CASES[case][2]
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
    again = eng.eval_factors()
    assert again[0] is Pf and again[1] is Qf                 # rebuilt only after a step
    Vt = eng.V.cpu().numpy()
    assert (Vt < 0).any() and np.array_equal(Qf.cpu().numpy(), np.where(Vt > 0, Vt, np.float32(0)))
    assert Qf.data_ptr() != eng.V.data_ptr()
    full = predict_scores(Pf, Qf, users.tolist(), None)
    assert np.abs(full - w64).max() <= bound
    got_c = predict_scores(Pf, Qf, users.tolist(), [c.tolist() for c in cand])
    c64, c32 = g["predict_cand_f64"], g["predict_cand_f32"]
    assert np.abs(np.stack(got_c) - c64).max() <= 4 * np.abs(c32 - c64).max() + 1e-5 * np.abs(c64).max()
    assert all(np.array_equal(r, full[k][c]) for k, (r, c) in enumerate(zip(got_c, cand)))
    # the empty user and every user with fewer than L items, against the restatement on the engine's own tables
    Pt, Vt, Wt = _tables(eng)
    short = np.asarray([u for u in range(U) if len(seqs.get(u, [])) < L], np.int32)
    assert any(u not in seqs for u in short.tolist()) and {len(seqs.get(u, [])) for u in short.tolist()} >= {0, 1, 2}
    want = P.predict(Pt, Vt, Wt, short, last)
    got_s = eng.score(short).cpu().numpy()
    assert np.abs(got_s - want).max() <= 1e-5 * np.abs(want).max()
    empty = int([u for u in short.tolist() if u not in seqs][0])
    k = short.tolist().index(empty)
    alone = np.maximum(Vt.astype(np.float64), 0) @ np.maximum(Pt[empty].astype(np.float64), 0)
    assert np.abs(got_s[k] - alone).max() <= 1e-5 * np.abs(want).max()
    _feed(eng, *_batch(g, case, 0), torch.zeros(2, device=eng.P.device))
    fresh = eng.eval_factors()
    assert fresh[0] is not Pf and fresh[1] is not Qf
    Vt = eng.V.cpu().numpy()
    assert np.array_equal(fresh[1].cpu().numpy(), np.where(Vt > 0, Vt, np.float32(0)))
    want = P.predict(*_tables(eng), short, last)                           # score() follows the step too
    assert np.abs(eng.score(short).cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    # L = 1: a context of one item, in training and in predict
    rs = np.random.RandomState(5)
    I = int(g["shape"][1])
    e1 = NPEEngine(g["P_0"], g["V_0"], g["W_0"], 0.05, 0.01, 64, 1, loss="square", learner="gd",
                   last_items=last_items_table(seqs, U, 1))
    st = P.State(g["P_0"], g["V_0"], g["W_0"], learner="gd", lr=0.05)
    loss2 = torch.zeros(2, device=e1.P.device)
    for _ in range(2):
        b = _random_batch(rs, U, I, 64, 1)
        got1, want1 = _feed(e1, *b, loss2), P.step(st, *b, "square", 0.01)
        assert abs(got1 - want1) <= 1e-5 * abs(want1)
    every = np.arange(U, dtype=np.int32)
    want = P.predict(*_tables(e1), every, P.last_items_table(seqs, U, 1))
    assert np.abs(e1.score(every).cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()


def _tables0(U, I, d, seed, scale=0.1):
    rs = np.random.RandomState(seed)
    return [(scale * rs.randn(n, d)).astype(np.float32) for n in (U, I, I)]


def _random_batch(rs, U, I, B, L):
    users = rs.randint(U, size=B).astype(np.int32)
    recents = rs.randint(I, size=(B, L)).astype(np.int32)
    items = rs.randint(I, size=B).astype(np.int32)
    return users, recents, items, (rs.rand(B) < 0.4).astype(np.float32)


def _against_restatement(tabs, batches, L, loss, lr, reg=0.01, learner="gd", max_batch=None):
    """the engine and the float64 restatement fed the same batches: loss and tables within 1e-5 max|want| after every
    step (fp32 storage of the tables and fp32 loss sums; FPMC's and HRM's bound).  The learner is plain gradient
    descent with a large step: the update is linear in the gradient, so a wrong or missing term of any gradient — a
    gate left open, a regulariser counted once — shows at its full size"""
    import torch
    from neurec_amd.npe import NPEEngine
    eng = NPEEngine(*tabs, lr, reg, max_batch or max(len(b[0]) for b in batches), L, loss=loss, learner=learner)
    st = P.State(*tabs, learner=learner, lr=lr)
    loss2 = torch.zeros(2, device=eng.P.device)
    for k, b in enumerate(batches):
        got = _feed(eng, *b, loss2)
        want = P.step(st, *b, loss, reg)
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
        for name, t in zip(P.TABLES, _tables(eng)):
            err = np.abs(t - st.var[name]).max()
            assert err <= 1e-5 * np.abs(st.var[name]).max(), (name, k, err)
    return eng, st


EDGES = [(d, 16) for d in (1, 16, 20, 64, 128)] + [(20, L) for L in (1, 2, 3)]


@pytest.mark.parametrize("loss", ["cross_entropy", "square"])
@pytest.mark.parametrize("d,L", EDGES)
def test_edges_against_the_float64_restatement(d, L, loss):
    """every lane layout (d = 1, 16, 20, 64, 128) at L = 16, L = 1, 2, 3 at d = 20 and both losses, with batches of 1,
    33, and 64 followed by a short last batch of 7, two gd steps each: 23 users and 31 items, the recents drawn with
    randint, so at L = 16 most instances hold an item twice and every batch but the first holds rows many times over
    in every role"""
    U, I = 23, 31
    scale = 0.5 if d == 1 else 0.3 if d <= 20 else 0.1
    twice = total = 0
    for sizes in ((1, 1), (33, 33), (64, 7)):
        rs = np.random.RandomState(1000 * d + 10 * L + sizes[0])
        batches = [_random_batch(rs, U, I, B, L) for B in sizes]
        twice += sum(len(set(r)) < L for b in batches for r in b[1].tolist())
        total += sum(sizes)
        _against_restatement(_tables0(U, I, d, d, scale), batches, L, loss, 0.25)
    assert L < 16 or 2 * twice > total


def test_constructed_gates_are_exact():
    """Two instances on dyadic tables, square loss, reg = 0, one gd step at lr = 1/4.  Instance 0 is (user 0, recents
    0 1 2, target 5, label 1), instance 1 (user 1, recents 1 1 3, target 0, label 0).  The columns: 0: P[0] = 0;
    1: V[5] = 0; 2: the context of instance 0 cancels (0.25 - 0.25 + 0); 3: P[1] = -0.0 and a negative context in
    instance 1; 4: a negative context with positive members in instance 0 (0.5 - 1 + 0.25); 5: V[5] negative.  Item 1
    stands twice among the recents of instance 1; item 0 is a recent in instance 0 and the target of instance 1.
    Every product and update is exact in fp32: the restatement run in float32 equals the float64 one exactly
    (checked first), the device equals both bit for bit, and the gated-off entries are exactly unchanged."""
    Pt = np.array([[0.0, 0.5, 0.25, 1.0, 0.5, 0.25], [0.5, 0.25, 0.5, -0.0, 0.25, 1.0], [3.0] * 6], np.float32)
    V = np.array([[0.5, 0.25, 1.0, 0.5, 0.25, 0.5], [1.0] * 6, [1.0] * 6, [1.0] * 6, [1.0] * 6,
                  [1.0, 0.0, 0.5, 0.25, 0.5, -0.5]], np.float32)
    W = np.array([[0.25, 0.5, 0.25, 0.5, 0.5, 0.25], [0.5, 0.25, -0.25, 0.25, -1.0, 0.5],
                  [0.25, 0.25, 0.0, 0.25, 0.25, 0.25], [-0.5, 0.5, 1.0, -1.0, 4.0, 0.25], [2.0] * 6, [2.0] * 6],
                 np.float32)
    users, recents = np.array([0, 1], np.int32), np.array([[0, 1, 2], [1, 1, 3]], np.int32)
    items, labels = np.array([5, 0], np.int32), np.array([1.0, 0.0], np.float32)
    lr = 0.25
    out = {}
    for dt in (np.float32, np.float64):
        tabs = [t.astype(dt) for t in (Pt, V, W)]
        loss, *G = P.gradients(*tabs, users, recents, items, labels, "square", 0.0)
        out[dt] = (loss, [t - dt(lr) * gr for t, gr in zip(tabs, G)], G)
    l64, new64, (GP, GV, GW) = out[np.float64]
    assert out[np.float32][0] == l64 == 13.015625                  # x = 1.875 and 3.5: g = 1.75 and 7
    for a, b in zip(out[np.float32][1], new64):
        assert np.array_equal(a.astype(np.float64), b) and np.array_equal(b.astype(np.float32), b)
    # the gradients themselves
    assert GP.tolist() == [[0.0, 0.0, 0.875, 0.4375, 0.875, 0.0], [3.5, 1.75, 7.0, 0.0, 1.75, 3.5], [0.0] * 6]
    assert GV[5].tolist() == [1.75, 0.0, 0.4375, 3.5, 0.875, 0.0]
    assert GV[0].tolist() == [7.0, 8.75, 7.0, 0.0, 15.75, 15.75] and not GV[1:5].any()
    assert GW[0].tolist() == GW[2].tolist() == [1.75, 0.0, 0.0, 0.4375, 0.0, 0.0]
    assert GW[1].tolist() == [1.75 + 7.0, 3.5, 14.0, 0.4375, 3.5, 7.0]           # once there, twice here
    assert GW[3].tolist() == [3.5, 1.75, 7.0, 0.0, 1.75, 3.5] and not GW[4:].any()
    import torch
    from neurec_amd.npe import NPEEngine
    eng = NPEEngine(Pt, V, W, lr, 0.0, 2, 3, loss="square", learner="gd")
    loss2 = torch.zeros(2, device=eng.P.device)
    got = _feed(eng, users, recents, items, labels, loss2)
    assert got == l64 and loss2.cpu().numpy().tolist() == [13.015625, 0.0]
    dev = _tables(eng)
    for name, t, want in zip(P.TABLES, dev, new64):
        assert np.array_equal(t, want.astype(np.float32)), name
    # the entries whose gate is shut are exactly what they were
    shut = {"P": [(0, 0), (0, 1), (0, 5), (1, 3)], "V": [(5, 1), (5, 5), (0, 3)],
            "W": [(0, 2), (2, 2), (0, 4), (0, 1), (2, 4), (3, 3)]}
    for name, t, was in zip(P.TABLES, dev, (Pt, V, W)):
        for r, c in shut[name]:
            assert t[r, c] == was[r, c], (name, r, c)
        assert (t != was).any()


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
    _against_restatement(_tables0(U, I, 20, 5), batches, L, "square", 0.02)


def test_one_batch_beyond_the_one_workgroup_sort():
    """The step's one internal capacity is the sort of its B (L + 2) keys: one workgroup's LDS network up to 16,384
    keys, the segmented multi-workgroup network beyond.  The smallest batch whose keys exceed it at L = 2 (4,097 slots:
    16,388 keys), against the restatement at d = 16, one step; every other test takes the first path."""
    L = 2
    B = SORT_ONE_WORKGROUP // (L + 2) + 1
    assert (L + 2) * (B - 1) <= SORT_ONE_WORKGROUP < (L + 2) * B
    rs = np.random.RandomState(2)
    U, I = 900, 1100
    _against_restatement(_tables0(U, I, 16, 6), [_random_batch(rs, U, I, B, L)], L, "square", 0.05)


def test_slots_that_take_no_part():
    """a user id >= U (or negative) and an item or any one recent outside [0, I): the slot takes no part — two gd steps
    give the loss and tables of the restatement fed the same batches without those slots (square: a sum over the
    instances)"""
    import torch
    from neurec_amd.npe import NPEEngine
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
    eng = NPEEngine(*tabs, 0.25, 0.01, B, L, loss="square", learner="gd")
    st = P.State(*tabs, learner="gd", lr=0.25)
    loss2 = torch.zeros(2, device=eng.P.device)
    for k in range(2):
        got = _feed(eng, *fed[k], loss2)
        want = P.step(st, *kept[k], "square", 0.01)
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
        for name, t in zip(P.TABLES, _tables(eng)):
            err = np.abs(t - st.var[name]).max()
            assert err <= 1e-5 * np.abs(st.var[name]).max(), (name, k, err)


def test_an_empty_batch_is_empty_work():
    """batch == 0: the loss kernel writes two zeros and no table moves"""
    import torch
    from neurec_amd.npe import NPEEngine
    tabs = _tables0(5, 6, 4, 1)
    eng = NPEEngine(*tabs, 0.1, 0.01, 8, 2, loss="square", learner="gd")
    dev = eng.P.device
    loss2 = torch.ones(2, device=dev)
    i32 = torch.zeros(0, dtype=torch.int32, device=dev)
    eng.step(i32, i32, i32, torch.zeros(0, device=dev), loss2)
    assert loss2.cpu().numpy().tolist() == [0.0, 0.0] and eng.t == 1
    assert all(np.array_equal(t, w) for t, w in zip(_tables(eng), tabs))


def test_row_gradients_are_stored_not_added(golden):
    """`gradients` alone, twice on the same batch with no application between: the head of a run STORES the row's sum,
    so the second call leaves the buffers bit for bit as the first did, rows the batch did not look up stay zero, and
    the buffers are the restatement's gradients (1e-5 max|want|)"""
    import torch
    g = golden
    case = "square_gd"
    eng = _engine(g, case)
    dev = eng.P.device
    b = _batch(g, case, 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    args = (t(b[0], torch.int32), t(b[1], torch.int32), t(b[2], torch.int32), t(b[3], torch.float32))
    loss2 = torch.zeros(2, device=dev)
    eng.gradients(*args, loss2)
    first = [eng.G[k].clone() for k in P.TABLES]
    eng.gradients(*args, loss2)
    assert all(torch.equal(eng.G[k], f) for k, f in zip(P.TABLES, first))
    _, *want = P.gradients(*(g[k + "_0"].astype(np.float64) for k in P.TABLES), *b, "square", float(g["reg"]))
    for k, f, w, looked in zip(P.TABLES, first, want, (b[0], b[2], b[1])):
        f = f.cpu().numpy()
        assert np.abs(f - w).max() <= 1e-5 * np.abs(w).max(), k
        assert not f[np.setdiff1d(np.arange(len(f)), looked.reshape(-1))].any(), k


@pytest.mark.parametrize("case", ["square_adam", "square_momentum"])
def test_two_engines_end_byte_identical(golden, case):
    """the same three batches twice (the cases of two steps: the first batch again as the third)"""
    import torch
    g = golden
    out = []
    for _ in range(2):
        eng = _engine(g, case)
        loss2 = torch.zeros(2, device=eng.P.device)
        n = len(g[case + "_users"])
        losses = [_feed(eng, *_batch(g, case, k % n), loss2) for k in range(3)]
        out.append([getattr(eng, k).clone() for k in P.TABLES] + [losses])
    assert all(torch.equal(a, b) for a, b in zip(out[0][:3], out[1][:3])) and out[0][3] == out[1][3]


def test_engine_refusals():
    import torch
    from neurec_amd.npe import NPEEngine
    z = lambda n, d=4: np.zeros((n, d), np.float32)
    with pytest.raises(NotImplementedError, match="128"):
        NPEEngine(z(5, 129), z(6, 129), z(6, 129), 0.01, 0.0, 8, 2)
    with pytest.raises(NotImplementedError, match="embedding_size=0"):
        NPEEngine(z(5, 0), z(6, 0), z(6, 0), 0.01, 0.0, 8, 2)
    with pytest.raises(NotImplementedError, match="high_order=0 is not supported \\(1 to 16\\)"):
        NPEEngine(z(5), z(6), z(6), 0.01, 0.0, 8, 0)
    with pytest.raises(NotImplementedError, match="high_order=17 is not supported \\(1 to 16\\)"):
        NPEEngine(z(5), z(6), z(6), 0.01, 0.0, 8, 17)
    with pytest.raises(Exception, match="please choose a suitable loss function"):
        NPEEngine(z(5), z(6), z(6), 0.01, 0.0, 8, 2, loss="bpr")
    with pytest.raises(ValueError, match="please select a suitable optimizer"):
        NPEEngine(z(5), z(6), z(6), 0.01, 0.0, 8, 2, learner="lbfgs")
    with pytest.raises(ValueError, match="V and W"):
        NPEEngine(z(5), z(6), z(7), 0.01, 0.0, 8, 2)
    eng = NPEEngine(z(5), z(6), z(6), 0.01, 0.0, 8, 2, loss="square")
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
    with pytest.raises(ValueError, match="last items"):
        eng.eval_factors()
    assert eng.t == 0 and not eng.G["W"].any().item()


# ------------------------------------------------------------------ drop-in
def _run(tmp_path, argv):
    from neurec_amd.main import main
    path = defaults.write_default_configs(str(tmp_path), overrides={
        "data.input.path": os.path.join(str(tmp_path), "dataset"), "data.input.dataset": "toy",
        "test_batch_size": "64", "by_time": "True"}, model_overrides={"NPE": {"embedding_size": "16"}})
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return main(argv=argv, properties=path)
    finally:
        os.chdir(cwd)


def test_npe_config_drops_in(tmp_path, monkeypatch):
    """NeuRec.properties + conf/NPE.properties (the reference's values, at embedding_size 16) + a UIRT file with
    by_time=True: two epochs through neurec_amd.main; the reference's log lines and the deviation line; the epoch-1
    loss against the restatement on the same stream, over the number of BATCHES (1e-4: the line carries six decimals
    of a loss near 0.7, and the engine's loss sums are fp32); the evaluation through the factor path, its metrics
    against the host's on predict() (1e-6, the bound test_hrm_config_drops_in holds)"""
    from test_fpmc_gpu import _host_metrics, _write_dataset
    from neurec_amd.data import TimeOrderPointwiseSampler
    from neurec_amd.model.sequential_recommender.NPE import DEVIATIONS
    from neurec_amd.util.tool import get_initializer
    _write_dataset(str(tmp_path))
    model = _run(tmp_path, ["--recommender=NPE", "--epochs=2"])
    folder = os.path.join(str(tmp_path), "log", "toy", "NPE")
    files = os.listdir(folder)
    assert len(files) == 1 and files[0].startswith("toy_NPE_")
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "NPE's hyperparameters:" in text and DEVIATIONS in text
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
    it = TimeOrderPointwiseSampler(ds, high_order=3, neg_num=4, batch_size=256, shuffle=True, as_tensors=True)
    init = get_initializer("tnormal", 0.01, seed=2017)
    st = P.State(init([ds.num_users, 16]), init([ds.num_items, 16]), init([ds.num_items, 16]), learner="adam",
                 lr=0.001)
    total = 0.0
    for users, recent, items, labels in it:
        total += P.step(st, users.cpu().numpy(), recent.reshape(-1, 3).cpu().numpy(), items.cpu().numpy(),
                        labels.cpu().numpy(), "cross_entropy", 0.1)
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
        _run(tmp_path, ["--recommender=NPE", "--epochs=1", "--loss_function=bpr"])        # not a pointwise loss
    with pytest.raises(ValueError, match="suitable optimizer"):
        _run(tmp_path, ["--recommender=NPE", "--epochs=1", "--learner=lbfgs"])
    with pytest.raises(NotImplementedError, match="128"):
        _run(tmp_path, ["--recommender=NPE", "--epochs=1", "--embedding_size=129"])
    with pytest.raises(NotImplementedError, match="1 to 16"):
        _run(tmp_path, ["--recommender=NPE", "--epochs=1", "--high_order=17"])
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)                                # WORLD_SIZE > 1
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(tmp_path, ["--recommender=NPE", "--epochs=1"])
