"""TransRec on the GPU (csrc/transrec.hip through neurec_amd/transrec.py): every step of the reference class's trace,
predict(), the edge shapes, the G_T chunking, long runs, one item in three roles, stored gradients, slots that take no
part and the sort's second path against the float64 restatement, determinism, the direct-difference scoring kernel's
edges and planted exact distances, the refusals and the drop-in run through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from neurec_amd import defaults
import transrec_restatement as P
from transrec_restatement import CASES

pytestmark = pytest.mark.gpu

SORT_ONE_WORKGROUP = 16384          # keys nrhip_sort_u64 sorts in one workgroup's LDS (csrc/bpr.hip: kPlanMaxKeys)
# gd steps of the edge tests.  "Large" is against the bound: a gradient term of size 0.1 moves a table by 5e-3, a
# thousand times the 1e-5 max|want| allowed; larger steps only blow the squared-distance scores up
LR = 0.05


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_transrec")


def _engine(g, case, **kw):
    from neurec_amd.transrec import TransRecEngine
    loss, learner, pairwise, reg = CASES[case]
    return TransRecEngine(g["P_0"], g["Q_0"], g["b_0"], g["T_0"], float(g["learning_rate"]), reg, 64, loss=loss,
                          pairwise=pairwise, learner=learner, **kw)


def _dev(eng, users, recent, items, third):
    import torch
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(eng.P.device, dt)
    return (t(users, torch.int32), t(recent, torch.int32), t(items, torch.int32),
            t(third, torch.int32 if eng.pairwise else torch.float32))


def _feed(eng, users, recent, items, third, loss2):
    eng.step(*_dev(eng, users, recent, items, third), loss2)
    return float(loss2.cpu().numpy().astype(np.float64).sum())


def _tables(eng):
    return [getattr(eng, k).cpu().numpy() for k in P.TABLES]


def _batch(g, case, k):
    return tuple(g["%s_%s" % (case, f)][k] for f in ("users", "recent", "items", "third"))


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Tables and loss after every step against the f64 trace: within 4x the reference's own f32-to-f64 distance of
    that step and table (read from the golden) plus 1e-5 max|want|.  Rows of P, Q and b outside <case>_rows_* are
    bit-equal to their initial value; the gradient buffers are zero again afterwards."""
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
            assert got.shape == w64.shape and err <= 4 * bar + 1e-5 * np.abs(w64).max(), (case, k, name, err, bar)
            if name != "T":
                still = np.setdiff1d(np.arange(len(got)), g["%s_rows_%s" % (case, name)])
                assert len(still) and np.array_equal(got[still], g[name + "_0"][still]), (case, k, name)
    for name in P.TABLES:                                     # the gradient buffers are zero again
        assert not eng.G[name].any().item(), name


def test_predict_matches_the_reference(golden):
    """full and candidate mode after the trained case `ce_adam`, under the trace's rule; a user with no train items
    scores b - |P_u + T - Q|"""
    import torch
    g = golden
    users, cand = g["predict_users"], g["predict_cand"]
    last = P.last_items(P.sequences(g), int(g["shape"][0]))
    eng = _engine(g, P.PREDICT_CASE)
    loss2 = torch.zeros(2, device=eng.P.device)
    for k in range(len(g[P.PREDICT_CASE + "_users"])):
        _feed(eng, *_batch(g, P.PREDICT_CASE, k), loss2)
    w64, w32 = g["predict_f64"], g["predict_f32"]
    got = eng.score(users, last).cpu().numpy().astype(np.float64)
    print("predict: device err %.3g, reference f32 err %.3g" % (np.abs(got - w64).max(), np.abs(w32 - w64).max()))
    assert got.shape == w64.shape
    assert np.abs(got - w64).max() <= 4 * np.abs(w32 - w64).max() + 1e-5 * np.abs(w64).max()
    got_c = np.stack([got[k][c] for k, c in enumerate(cand)])
    c64, c32 = g["predict_cand_f64"], g["predict_cand_f32"]
    print("predict, candidates: device err %.3g, reference f32 err %.3g" % (np.abs(got_c - c64).max(),
                                                                          np.abs(c32 - c64).max()))
    assert np.abs(got_c - c64).max() <= 4 * np.abs(c32 - c64).max() + 1e-5 * np.abs(c64).max()
    empty = int(np.flatnonzero(last < 0)[0])
    Pm, Q, b, T = (t.astype(np.float64) for t in _tables(eng))
    want = b - np.sqrt(((Pm[empty] + T - Q) ** 2).sum(axis=1))
    got_e = eng.score(np.asarray([empty], np.int32), last).cpu().numpy()[0]
    assert np.abs(got_e - want).max() <= 1e-5 * np.abs(want).max()


def _tables0(U, I, d, seed, scale=0.1):
    rs = np.random.RandomState(seed)
    return [(scale * rs.randn(*shape)).astype(np.float32) for shape in ((U, d), (I, d), (I,), (d,))]


def _random_batch(rs, U, I, B, pairwise):
    users = rs.randint(U, size=B).astype(np.int32)
    recent = rs.randint(I, size=B).astype(np.int32)
    items = rs.randint(I, size=B).astype(np.int32)
    third = rs.randint(I, size=B).astype(np.int32) if pairwise else (rs.rand(B) < 0.4).astype(np.float32)
    return users, recent, items, third


def _check_tables(eng, st, where):
    for name, t in zip(P.TABLES, _tables(eng)):
        err = np.abs(t - st.var[name]).max()
        assert err <= 1e-5 * np.abs(st.var[name]).max(), (name, where, err)


def _against_restatement(tabs, batches, pairwise, loss, lr=LR, reg=0.01, learner="gd", max_batch=None):
    """the engine and the float64 restatement fed the same batches: loss and tables within 1e-5 max|want| after every
    step (fp32 storage of O(0.1) tables and fp32 loss terms).  The learner is plain gradient descent: the update is
    linear in the gradient, so a wrong or missing term of any gradient shows at its full size"""
    import torch
    from neurec_amd.transrec import TransRecEngine
    eng = TransRecEngine(*tabs, lr, reg, max_batch or max(len(b[0]) for b in batches), loss=loss, pairwise=pairwise,
                         learner=learner)
    st = P.State(*tabs, learner=learner, lr=lr)
    loss2 = torch.zeros(2, device=eng.P.device)
    for k, b in enumerate(batches):
        got = _feed(eng, *b, loss2)
        want = P.step(st, *b, pairwise, loss, reg)
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
        _check_tables(eng, st, k)
    return eng, st


MODES = [("pair", "bpr"), ("pair", "hinge"), ("pair", "square"), ("point", "cross_entropy"), ("point", "square")]


@pytest.mark.parametrize("d", [1, 16, 20, 50, 64, 128])
@pytest.mark.parametrize("mode,loss", MODES)
def test_edges_against_the_float64_restatement(d, mode, loss):
    """every lane layout (d = 1, 16, 20, 50, 64, 128) crossed with batches of 1, 33, and 64 followed by a short last
    batch of 7, both modes and every loss, two gd steps each: 23 users and 31 items, so every batch but the first holds
    rows many times over in every role"""
    pairwise = mode == "pair"
    U, I = 23, 31
    scale = 0.5 if d == 1 else 0.3 if d <= 20 else 0.1
    for sizes in ((1, 1), (33, 33), (64, 7)):
        rs = np.random.RandomState(1000 * d + sizes[0])
        batches = [_random_batch(rs, U, I, B, pairwise) for B in sizes]
        _against_restatement(_tables0(U, I, d, d, scale), batches, pairwise, loss)


@pytest.mark.parametrize("pairwise", [False, True])
def test_batches_at_the_chunks_of_the_translation_gradient(pairwise):
    """G_T is summed per chunk of the batch, then over the chunks: one batch each at the chunk size, one more, and two
    chunks and three; reg = 0.5 so that a regulariser applied to T per instance or per chunk shows"""
    from neurec_amd.transrec import GT_CHUNK
    U, I, d = 23, 31, 20
    for B in (GT_CHUNK, GT_CHUNK + 1, 2 * GT_CHUNK + 3):
        rs = np.random.RandomState(B)
        _against_restatement(_tables0(U, I, d, 7, 0.3), [_random_batch(rs, U, I, B, pairwise)], pairwise,
                             "bpr" if pairwise else "square", reg=0.5)


@pytest.mark.parametrize("pairwise", [False, True])
def test_long_runs(pairwise):
    """U = 40, I = 50, d = 20, B = 128: one item is the target of 70 instances and the `recent` of 70 others (and,
    pairwise, the negative of 40), one user holds 70 instances — runs longer than a wavefront, one row in three roles"""
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
        if pairwise:
            third[rs.permutation(B)[:40]] = 11
            assert (third == 11).sum() >= 40
        batches.append((users, recent, items, third))
    _against_restatement(_tables0(U, I, 20, 5), batches, pairwise, "bpr" if pairwise else "square", lr=0.02)


@pytest.mark.parametrize("loss", ["bpr", "square"])
def test_one_item_in_three_roles(loss):
    """item 4 is a recent, a target and a negative in one batch, instance 3 has i == l, instance 5 has i == j and
    instance 6 all three equal; reg = 0.5, so a regulariser term given to the wrong role (or to the second inference's
    P_u / Q_l lookups) shows at half the row's size"""
    users = np.asarray([0, 1, 2, 3, 0, 4, 2, 1], np.int32)
    recent = np.asarray([4, 2, 7, 5, 4, 1, 4, 8], np.int32)
    items = np.asarray([1, 4, 3, 5, 6, 2, 4, 0], np.int32)
    third = np.asarray([8, 0, 4, 6, 4, 2, 4, 3], np.int32)
    pat = P.edge_patterns(users, recent, items, third, True)
    assert all(pat.values()) and recent[3] == items[3] and items[5] == third[5]
    rs = np.random.RandomState(1)
    second = _random_batch(rs, 5, 9, 8, True)
    _against_restatement(_tables0(5, 9, 16, 11, 0.3), [(users, recent, items, third), second], True, loss, reg=0.5)
    # the same instances pointwise: item 4 a recent and a target, instance 3 with i == l
    labels = np.asarray([1, 0, 1, 1, 0, 1, 0, 1], np.float32)
    _against_restatement(_tables0(5, 9, 16, 11, 0.3), [(users, recent, items, labels)], False, "square", reg=0.5)


@pytest.mark.parametrize("pairwise", [False, True])
def test_gradients_are_stored_not_added(pairwise):
    """gradients() on buffers pre-filled with garbage: the rows the batch touches hold the restatement's gradient, the
    others the garbage — and so does G_b of an item that appears as a recent item only; G_T is stored whole"""
    import torch
    from neurec_amd.transrec import TransRecEngine
    U, I, d, B = 61, 83, 20, 40
    rs = np.random.RandomState(77)
    users, recent, items, third = _random_batch(rs, U, I - 1, B, pairwise)
    recent[5] = I - 1                                         # item I - 1: a recent item, never a target or negative
    tabs = _tables0(U, I, d, 3, 0.3)
    loss = "bpr" if pairwise else "square"
    eng = TransRecEngine(*tabs, LR, 0.5, B, loss=loss, pairwise=pairwise, learner="gd")
    for k in P.TABLES:
        eng.G[k].fill_(7.0)
    loss2 = torch.zeros(2, device=eng.P.device)
    eng.gradients(*_dev(eng, users, recent, items, third), loss2)
    total, G = P.gradients(*[np.asarray(t, np.float64) for t in tabs], users, recent, items, third, pairwise, loss, 0.5)
    got_loss = float(loss2.cpu().numpy().astype(np.float64).sum())
    assert abs(got_loss - total) <= 1e-5 * abs(total)
    rows = P.touched(users, recent, items, third, pairwise)
    assert I - 1 in rows["Q"] and I - 1 not in rows["b"]
    for name in P.ROWS:
        got = eng.G[name].cpu().numpy()
        r = rows[name]
        assert np.abs(got[r] - G[name][r]).max() <= 1e-5 * np.abs(G[name][r]).max(), name
        rest = np.setdiff1d(np.arange(len(got)), r)
        assert len(rest) and np.all(got[rest] == 7.0), name
    got_T = eng.G["T"].cpu().numpy()
    assert np.abs(got_T - G["T"]).max() <= 1e-5 * np.abs(G["T"]).max()
    assert eng.t == 0 and all(np.array_equal(a, b.reshape(a.shape)) for a, b in zip(_tables(eng), tabs))


@pytest.mark.parametrize("pairwise", [False, True])
def test_one_batch_beyond_the_one_workgroup_sort(pairwise):
    """The step's one internal capacity is the sort of its 3 N keys: one workgroup's LDS network up to 16,384 keys,
    the segmented multi-workgroup network beyond.  The smallest batch whose keys exceed it, against the restatement at
    d = 16; this batch is also the one that takes the capped number of G_T chunks"""
    from neurec_amd.transrec import GT_CHUNK, GT_MAX_CHUNKS
    per = 6 if pairwise else 3
    B = SORT_ONE_WORKGROUP // per + 1
    assert per * (B - 1) <= SORT_ONE_WORKGROUP < per * B and B > GT_CHUNK * GT_MAX_CHUNKS
    rs = np.random.RandomState(2)
    U, I = 900, 1100
    batches = [_random_batch(rs, U, I, B, pairwise)]
    _against_restatement(_tables0(U, I, 16, 6), batches, pairwise, "bpr" if pairwise else "square")


@pytest.mark.parametrize("pairwise", [False, True])
def test_slots_that_take_no_part(pairwise):
    """a user id >= U (or negative) and an item, recent or negative outside [0, I): the slot takes no part — two gd
    steps give the loss and tables of the restatement fed the same batches without those slots (square / bpr: sums
    over the instances)"""
    import torch
    from neurec_amd.transrec import TransRecEngine
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
    tabs = _tables0(U, I, 16, 3, 0.3)
    loss = "bpr" if pairwise else "square"
    eng = TransRecEngine(*tabs, LR, 0.01, B, loss=loss, pairwise=pairwise, learner="gd")
    st = P.State(*tabs, learner="gd", lr=LR)
    loss2 = torch.zeros(2, device=eng.P.device)
    for k in range(2):
        got = _feed(eng, *fed[k], loss2)
        want = P.step(st, *kept[k], pairwise, loss, 0.01)
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
        _check_tables(eng, st, k)


@pytest.mark.parametrize("case", ["square_adam", "bpr_adam", "square_momentum"])
def test_two_engines_end_byte_identical(golden, case):
    """the same three batches twice (the cases of two steps: the first batch again as the third); T included"""
    import torch
    g = golden
    out = []
    for _ in range(2):
        eng = _engine(g, case)
        loss2 = torch.zeros(2, device=eng.P.device)
        n = len(g[case + "_users"])
        losses = [_feed(eng, *_batch(g, case, k % n), loss2) for k in range(3)]
        out.append([getattr(eng, k).clone() for k in P.TABLES] + [losses])
    assert all(torch.equal(a, b) for a, b in zip(out[0][:4], out[1][:4])) and out[0][4] == out[1][4]
    assert not torch.equal(out[0][3].cpu(), torch.from_numpy(g["T_0"].reshape(-1)))


def test_empty_work_is_accepted():
    import torch
    from neurec_amd.transrec import TransRecEngine
    tabs = _tables0(5, 6, 4, 1)
    eng = TransRecEngine(*tabs, 0.01, 0.1, 8, loss="square", pairwise=False)
    dev = eng.P.device
    i32 = torch.zeros(0, dtype=torch.int32, device=dev)
    loss2 = torch.ones(2, device=dev)
    eng.step(i32, i32, i32, torch.zeros(0, device=dev), loss2)
    assert loss2.tolist() == [0.0, 0.0] and eng.t == 0
    assert all(np.array_equal(a, b) for a, b in zip(_tables(eng), tabs))
    last = np.zeros(5, np.int32)
    assert tuple(eng.score(np.zeros(0, np.int32), last).shape) == (0, 6)
    assert tuple(eng.queries(last, np.zeros(0, np.int32)).shape) == (0, 4)
    none = TransRecEngine(tabs[0], np.zeros((0, 4), np.float32), np.zeros(0, np.float32), tabs[3], 0.01, 0.1, 8)
    assert tuple(none.score(np.arange(3, dtype=np.int32), np.full(5, -1, np.int32)).shape) == (3, 0)


# ------------------------------------------------------------------ the scoring kernel
@pytest.mark.parametrize("d", [1, 20, 50, 64, 128])
def test_scores_at_the_edges_of_the_tile(d):
    """n = 1, 63, 65 users (shuffled, one of them twice) against I = 1, 63, 64, 65, 200 items: output tiles of 64 x 64
    cut on either side, columns staged 32 at a time cut by d; every fourth user without a recent item.  Written into a
    buffer wider than I, whose columns beyond I stay as they were"""
    import torch
    from neurec_amd.transrec import TransRecEngine
    U = 70
    for I in (1, 63, 64, 65, 200):
        tabs = _tables0(U, I, d, 10 * d + I, 0.3)
        eng = TransRecEngine(*tabs, 0.01, 0.0, 8)
        rs = np.random.RandomState(I)
        last = rs.randint(I, size=U).astype(np.int32)
        last[::4] = -1
        for n in (1, 63, 65):
            users = rs.permutation(U)[:n].astype(np.int32)
            if n > 1:
                users[n // 2] = users[0]
            want = P.predict(*tabs, users, last)
            out = torch.full((n, I + 7), -3.0, device=eng.P.device)
            q = eng.queries(last, users)
            assert eng.score_queries(q, out) is out
            got = out.cpu().numpy()
            assert np.abs(got[:, :I] - want).max() <= 1e-5 * np.abs(want).max(), (d, I, n)
            assert np.all(got[:, I:] == -3.0)
            assert torch.equal(eng.score(users, last), out[:, :I])


def test_planted_exact_distances():
    """Dyadic tables around 1 (multiples of 1/64 in [0.5, 1.5]) at d = 50: the query P_u + T + Q_last is exact in fp32.
    An item whose row IS the query scores exactly its bias (not NaN); an item whose row differs from the query by 2^-12
    in one column scores exactly bias - 2^-12.  Only the direct form (subtract, then multiply-accumulate) gives these
    bits: |q|^2 and |Q_j|^2 are about 450, whose fp32 spacing (3e-5) is five hundred times the 2^-24 that the expanded
    form |q|^2 + |Q_j|^2 - 2 q.Q_j would have to resolve"""
    from neurec_amd.transrec import TransRecEngine
    rs = np.random.RandomState(12)
    U, I, d = 9, 130, 50
    dy = lambda *shape: (1.0 + rs.randint(-32, 33, size=shape) / 64.0).astype(np.float32)
    Pm, Q, T = dy(U, d), dy(I, d), dy(d)
    b = (rs.randint(-64, 65, size=I) / 64.0).astype(np.float32)
    last = rs.randint(3, size=U).astype(np.int32)               # recents among items 0..2, planted rows beyond
    users = np.asarray([4, 7, 1], np.int32)
    q = Pm[users] + T + Q[last[users]]
    assert np.array_equal(q.astype(np.float64), Pm[users].astype(np.float64) + T + Q[last[users]])      # exact
    same, near = [10, 77, 129], [11, 64, 128]
    step = np.float32(2.0 ** -12)
    for k in range(3):
        Q[same[k]] = q[k]
        Q[near[k]] = q[k]
        Q[near[k], 7 * k + 3] += step if k != 1 else -step
        assert Q[near[k], 7 * k + 3] != q[k, 7 * k + 3]
    eng = TransRecEngine(Pm, Q, b, T, 0.01, 0.0, 8)
    got = eng.score(users, last).cpu().numpy()
    assert np.all(np.isfinite(got))
    for k in range(3):
        assert got[k, same[k]] == b[same[k]], (k, got[k, same[k]], b[same[k]])
        assert got[k, near[k]] == np.float32(b[near[k]] - step), (k, got[k, near[k]], b[near[k]])
        # what the expanded form gives in fp32 on the same rows: it cannot hold the planted 2^-24
        qq, jj = np.float32(np.dot(q[k], q[k])), np.float32(np.dot(Q[near[k]], Q[near[k]]))
        expanded = np.float32(qq + jj - np.float32(2) * np.float32(np.dot(q[k], Q[near[k]])))
        assert expanded != np.float32(2.0 ** -24)
    want = P.predict(Pm, Q, b, T, users, last)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


# ------------------------------------------------------------------ refusals
def test_engine_refusals():
    import torch
    from neurec_amd.transrec import TransRecEngine
    z = lambda *shape: np.zeros(shape, np.float32)
    with pytest.raises(NotImplementedError, match="1 to 128"):
        TransRecEngine(z(5, 129), z(6, 129), z(6), z(129), 0.01, 0.0, 8)
    with pytest.raises(Exception, match="please choose a suitable loss function"):
        TransRecEngine(z(5, 4), z(6, 4), z(6), z(4), 0.01, 0.0, 8, loss="hinge", pairwise=False)
    with pytest.raises(Exception, match="please choose a suitable loss function"):
        TransRecEngine(z(5, 4), z(6, 4), z(6), z(4), 0.01, 0.0, 8, loss="cross_entropy", pairwise=True)
    with pytest.raises(ValueError, match="please select a suitable optimizer"):
        TransRecEngine(z(5, 4), z(6, 4), z(6), z(4), 0.01, 0.0, 8, learner="lbfgs")
    with pytest.raises(ValueError, match="embedding_size"):
        TransRecEngine(z(5, 4), z(6, 3), z(6), z(4), 0.01, 0.0, 8)
    with pytest.raises(ValueError, match="num_items entries"):
        TransRecEngine(z(5, 4), z(6, 4), z(5), z(4), 0.01, 0.0, 8)
    with pytest.raises(ValueError, match="embedding_size entries"):
        TransRecEngine(z(5, 4), z(6, 4), z(6), z(3), 0.01, 0.0, 8)
    eng = TransRecEngine(z(5, 4), z(6, 4), z(6), z(1, 4), 0.01, 0.0, 8, loss="square", pairwise=False)
    dev = eng.P.device
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    loss2 = torch.zeros(2, device=dev)
    with pytest.raises(ValueError, match="max_batch"):
        eng.step(i32(9), i32(9), i32(9), torch.zeros(9, device=dev), loss2)
    with pytest.raises(ValueError, match="same length"):
        eng.step(i32(4), i32(3), i32(4), torch.zeros(4, device=dev), loss2)
    with pytest.raises(ValueError, match="same length"):
        eng.step(i32(4), i32(4), i32(4), torch.zeros(5, device=dev), loss2)
    with pytest.raises(ValueError, match="last_items holds 4 entries"):
        eng.score(np.arange(2, dtype=np.int32), np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="queries must be"):
        eng.score_queries(torch.zeros((2, 5), device=dev))
    with pytest.raises(ValueError, match="out must be"):
        eng.score_queries(torch.zeros((2, 4), device=dev), torch.zeros((2, 5), device=dev))
    assert eng.t == 0 and not any(eng.G[k].any().item() for k in P.TABLES)


# ------------------------------------------------------------------ drop-in
def _run(tmp_path, argv):
    from neurec_amd.main import main
    path = defaults.write_default_configs(str(tmp_path), overrides={
        "data.input.path": os.path.join(str(tmp_path), "dataset"), "data.input.dataset": "toy",
        "test_batch_size": "64", "by_time": "True"}, model_overrides={"TransRec": {"learning_rate": "0.01"}})
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return main(argv=argv, properties=path)
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("pairwise", [True, False])
def test_transrec_config_drops_in(tmp_path, pairwise):
    """NeuRec.properties + conf/TransRec.properties (the reference's values, at learning_rate 0.01 so that two epochs
    show) + a UIRT file with by_time=True: two epochs through neurec_amd.main in both modes; the reference's log lines —
    no `[iter ...]` line, which the reference comments out — and the deviation line, in order; the loss finite and
    lower in epoch 2; the metric columns against the host's metrics on engine.score rows (1e-6)"""
    from test_fpmc_gpu import _host_metrics, _write_dataset
    from neurec_amd.model.sequential_recommender.TransRec import NO_HISTORY
    _write_dataset(str(tmp_path))
    argv = ["--recommender=TransRec", "--epochs=2"]
    if not pairwise:
        argv += ["--is_pairwise=False", "--loss_function=cross_entropy"]
    model = _run(tmp_path, argv)
    assert model.engine.pairwise is pairwise and model.engine.d == 50
    folder = os.path.join(str(tmp_path), "log", "toy", "TransRec")
    files = os.listdir(folder)
    assert len(files) == 1 and files[0].startswith("toy_TransRec_")
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "TransRec's hyperparameters:" in text and "[iter" not in text
    lines = [ln for ln in text.splitlines() if re.search(r"metrics:\t|epoch \d+:\t", ln) or NO_HISTORY in ln]
    kinds = ["m" if "metrics:" in ln else "d" if NO_HISTORY in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)
             for ln in lines]
    assert kinds == ["m", "d", "e1", "e2"], kinds                         # no evaluation before the first epoch
    losses = model.epoch_losses                                           # per epoch, over the number of batches
    assert len(losses) == 2 and np.all(np.isfinite(losses)) and losses[1] < losses[0], losses
    evals = re.findall(r"epoch (\d+):\t(.+)", text)
    shown = np.asarray([float(x) for x in evals[-1][1].split()])
    assert np.all(np.isfinite(shown)) and shown.max() > 0
    uni = model.evaluator.evaluator
    users = list(uni.user_pos_test.keys())
    scores = model.engine.score(np.asarray(users, np.int32), model.last_items).cpu().numpy()
    assert scores.shape == (len(users), model.num_items) and scores.dtype == np.float32
    host = _host_metrics(scores, uni.user_pos_train, uni.user_pos_test, users, uni.top_show, uni.metrics)
    print("metrics: evaluator %s\n         host      %s" % (shown, host))
    assert np.abs(host - shown).max() <= 1e-6
    full = model.predict([0, 5, 9], None)
    assert tuple(full.shape) == (3, model.num_items) and full.is_cuda
    full = full.cpu().numpy()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])
    assert np.array_equal(cand[1], full[1][[7]])


def test_refusals(tmp_path, monkeypatch):
    from test_fpmc_gpu import _write_dataset
    _write_dataset(str(tmp_path))
    with pytest.raises(Exception, match="suitable loss function"):
        _run(tmp_path, ["--recommender=TransRec", "--epochs=1", "--loss_function=cross_entropy"])   # pairwise mode
    with pytest.raises(ValueError, match="suitable optimizer"):
        _run(tmp_path, ["--recommender=TransRec", "--epochs=1", "--learner=lbfgs"])
    with pytest.raises(NotImplementedError, match="1 to 128"):
        _run(tmp_path, ["--recommender=TransRec", "--epochs=1", "--embedding_size=129"])
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)                                # WORLD_SIZE > 1
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(tmp_path, ["--recommender=TransRec", "--epochs=1"])
