"""FPMCplus on the GPU (csrc/fpmcplus.hip through neurec_amd/fpmcplus.py): every step of the reference class's trace,
predict(), L = 1, the edge shapes, permuted recents, absent slots, stored-not-added row gradients, the sort's second
path, determinism and a long run against the restatement, the refusals and the drop-in run through neurec_amd.main.

Bounds.  Against the trace: 4 x the reference's own f32-to-f64 distance for that step and table (read from the fixture)
+ 1e-5 max|want|, the bound of every sibling.  Against the float64 restatement on shapes the trace does not hold:
1e-5 max|want| — the tables are stored in fp32 (2^-24 relative per stored value) and every sum of the step is an fp32
sum of at most a few thousand terms; FPMC's, HRM's and NPE's tests hold the same figure."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from neurec_amd import defaults
import fpmcplus_restatement as P
from fpmcplus_restatement import CASES

pytestmark = pytest.mark.gpu

SORT_ONE_WORKGROUP = 16384          # keys nrhip_sort_u64 sorts in one workgroup's LDS (csrc/bpr.hip: kPlanMaxKeys)


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_fpmcplus")


def _new(tabs, lr, reg_mf, reg_w, max_batch, L, loss, pairwise, learner="gd", **kw):
    from neurec_amd.fpmcplus import FPMCplusEngine
    return FPMCplusEngine(*tabs, lr, reg_mf, reg_w, max_batch, L, loss=loss, pairwise=pairwise, learner=learner, **kw)


def _engine(g, case, **kw):
    loss, learner, pairwise, L = CASES[case]
    return _new(P.golden_tables(g, case, "f32", -1), float(g["learning_rate"]), float(g["reg_mf"]), float(g["reg_w"]),
                64, L, loss, pairwise, learner, **kw)


def _dev(eng, users, recents, items, third):
    import torch
    dev = eng.UI.device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    return (t(users, torch.int32), t(recents, torch.int32), t(items, torch.int32),
            t(third, torch.int32 if eng.pairwise else torch.float32))


def _feed(eng, users, recents, items, third, loss2):
    eng.step(*_dev(eng, users, recents, items, third), loss2)
    return float(loss2.cpu().numpy().astype(np.float64).sum())


def _tables(eng):
    return [getattr(eng, k).cpu().numpy() for k in P.TABLES]


def _batch(g, case, k):
    return tuple(g["%s_%s" % (case, f)][k] for f in ("users", "recents", "items", "third"))


def _train(eng, g, case):
    import torch
    loss2 = torch.zeros(2, device=eng.UI.device)
    return [_feed(eng, *_batch(g, case, k), loss2) for k in range(len(g[case + "_users"]))]


def _zero_G(eng):
    return all(not eng.G[k].any().item() for k in P.TABLES)


# ------------------------------------------------------------------ the trace
@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """the seven tables and the loss after every step against the f64 trace; rows outside <case>_rows_* are bit-equal
    to their initial value; every gradient buffer is zero afterwards"""
    import torch
    g = golden
    eng = _engine(g, case)
    init = P.golden_tables(g, case, "f32", -1)
    loss2 = torch.zeros(2, device=eng.UI.device)
    for k in range(len(g[case + "_users"])):
        loss = _feed(eng, *_batch(g, case, k), loss2)
        want, ref32 = g[case + "_f64_loss"][k], g[case + "_f32_loss"][k]
        print("%s step %d loss: device err %.3g, reference f32 err %.3g" % (case, k + 1, abs(loss - want),
                                                                           abs(ref32 - want)))
        assert abs(loss - want) <= 4 * abs(ref32 - want) + 1e-5 * abs(want)
        for name, got, t0, w64, w32 in zip(P.TABLES, _tables(eng), init, P.golden_tables(g, case, "f64", k),
                                           P.golden_tables(g, case, "f32", k)):
            bar = np.abs(w32.astype(np.float64) - w64).max()
            err = np.abs(got.astype(np.float64) - w64).max()
            print("%s step %d %s: device err %.3g, reference f32 err %.3g" % (case, k + 1, name, err, bar))
            assert err <= 4 * bar + 1e-5 * np.abs(w64).max(), (case, k, name, err, bar)
            if name in P.ROWS:
                still = np.setdiff1d(np.arange(len(got)), g["%s_rows_%s" % (case, name)])
                assert len(still) and np.array_equal(got[still], t0[still]), (case, k, name)
        assert _zero_G(eng)


def test_predict_matches_the_reference(golden):
    """full and candidate mode after the predict case; candidate entries are the full rows' entries; deviations (a)
    and (b): every user with |R_u| < L, an empty one among them, against the restatement on the engine's own tables"""
    from neurec_amd.fpmcplus import last_items_table
    g = golden
    case = P.PREDICT_CASE
    L = CASES[case][3]
    users, cand = g["predict_users"], g["predict_cand"]
    seqs = P.sequences(g)
    U = int(g["shape"][0])
    last = last_items_table(seqs, U, L)
    assert np.array_equal(last, P.last_items_table(seqs, U, L))
    eng = _engine(g, case, last_items=last)
    _train(eng, g, case)
    w64, w32 = g["predict_f64"], g["predict_f32"]
    bound = 4 * np.abs(w32 - w64).max() + 1e-5 * np.abs(w64).max()
    full = eng.score(users).cpu().numpy()
    print("predict: device err %.3g, reference f32 err %.3g" % (np.abs(full - w64).max(), np.abs(w32 - w64).max()))
    assert full.shape == w64.shape and np.abs(full - w64).max() <= bound
    c64, c32 = g["predict_cand_f64"], g["predict_cand_f32"]
    got_c = np.stack([full[k][c] for k, c in enumerate(cand)])
    assert np.abs(got_c - c64).max() <= 4 * np.abs(c32 - c64).max() + 1e-5 * np.abs(c64).max()
    # the plugin's predict() on these tables, full and candidate mode, against the reference's own rows
    from neurec_amd.model.sequential_recommender.FPMCplus import FPMCplus
    model = FPMCplus.__new__(FPMCplus)
    model.engine = eng
    full_p = model.predict(users.tolist(), None)
    assert np.array_equal(full_p.cpu().numpy(), full)
    cand_p = model.predict(users.tolist(), [c.tolist() for c in cand])
    assert np.abs(np.stack(cand_p) - c64).max() <= 4 * np.abs(c32 - c64).max() + 1e-5 * np.abs(c64).max()
    assert all(np.array_equal(r, full[k][c]) for k, (r, c) in enumerate(zip(cand_p, cand)))
    short = np.asarray([u for u in range(U) if len(seqs.get(u, [])) < L], np.int32)
    assert any(u not in seqs for u in short.tolist()) and {len(seqs.get(u, [])) for u in short.tolist()} >= {0, 1, 2}
    want = P.predict(*_tables(eng), short, last)
    got_s = eng.score(short).cpu().numpy()
    assert np.abs(got_s - want).max() <= 1e-5 * np.abs(want).max()
    empty = int([u for u in short.tolist() if u not in seqs][0])
    UI, IU = _tables(eng)[:2]
    alone = IU.astype(np.float64) @ UI[empty].astype(np.float64)
    assert np.abs(got_s[short.tolist().index(empty)] - alone).max() <= 1e-5 * np.abs(want).max()


# ------------------------------------------------------------------ against the restatement
def _tables0(U, I, d, w, seed, scale=0.1, h_ones=False):
    rs = np.random.RandomState(seed)
    tabs = [(scale * rs.randn(n, d)).astype(np.float32) for n in (U, I, I, I)]
    tabs.append((rs.randn(3 * d, w) / np.sqrt(3 * d)).astype(np.float32))
    tabs.append((0.1 * rs.randn(w)).astype(np.float32))
    tabs.append(np.ones(w, np.float32) if h_ones else (1.0 + 0.1 * rs.randn(w)).astype(np.float32))
    return tabs


def _random_batch(rs, U, I, B, L, pairwise):
    users = rs.randint(U, size=B).astype(np.int32)
    recents = rs.randint(I, size=(B, L)).astype(np.int32)
    items = rs.randint(I, size=B).astype(np.int32)
    third = rs.randint(I, size=B).astype(np.int32) if pairwise else (rs.rand(B) < 0.4).astype(np.float32)
    return users, recents, items, third


def _close(eng, st, what=""):
    for name, t in zip(P.TABLES, _tables(eng)):
        err = np.abs(t - st.var[name]).max()
        assert err <= 1e-5 * np.abs(st.var[name]).max(), (what, name, err)


def _against_restatement(tabs, batches, L, loss, pairwise, lr, reg_mf=0.01, reg_w=0.02, learner="gd", fed=None,
                         max_batch=None):
    """the engine fed `fed` (default: `batches`) and the float64 restatement fed `batches`: loss and the seven tables
    within 1e-5 max|want| after every step.  The learner is plain gradient descent with a large step: the update is
    linear in the gradient, so a wrong or missing term of any gradient shows at its full size"""
    import torch
    fed = batches if fed is None else fed
    eng = _new(tabs, lr, reg_mf, reg_w, max_batch or max(len(b[0]) for b in fed), L, loss, pairwise, learner)
    st = P.State(*tabs, learner=learner, lr=lr)
    loss2 = torch.zeros(2, device=eng.UI.device)
    for k, (b, f) in enumerate(zip(batches, fed)):
        got = _feed(eng, *f, loss2)
        want = P.step(st, *b, pairwise, loss, reg_mf, reg_w)
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
        _close(eng, st, k)
        assert _zero_G(eng)
    return eng, st


EDGES = [(d, 16, 3) for d in (1, 17, 64, 65, 128)] + [(17, w, 3) for w in (1, 33, 64)] + [(128, 64, 3), (64, 64, 3)] + \
        [(17, 16, L) for L in (1, 2, 5, 9, 16)]


@pytest.mark.parametrize("d,w,L", EDGES)
def test_edges_against_the_float64_restatement(d, w, L):
    """40 x 30 tables, B = 7 and B = 1, one gd step each, pairwise (bpr) and pointwise (square): every lane layout of
    the rows (d = 1, 17, 64, 65, 128), of the projections (w = 1, 16, 33, 64), the corners (128, 64) and (64, 64) — the
    largest item tile of either scoring instantiation — and L = 1, 2, 3, 5, 9, 16 (every padded order 1, 2, 4, 8, 16 of
    the scoring kernel, 9 with its upper half partly absent); then score() of every user (30 items: no multiple of the scoring tile), of one user, and of 300 users (two
    user blocks of the scoring kernel) against predict() of the restatement"""
    U, I = 40, 30
    scale = 0.5 if d == 1 else 0.3 if d <= 17 else 0.1
    rs = np.random.RandomState(1000 * d + 10 * w + L)
    for pairwise, loss in ((True, "bpr"), (False, "square")):
        tabs = _tables0(U, I, d, w, d + w, scale)
        for B in (7, 1):
            eng, st = _against_restatement(tabs, [_random_batch(rs, U, I, B, L, pairwise)], L, loss, pairwise, 0.25)
        last = np.where(rs.rand(U, L) < 0.8, rs.randint(I, size=(U, L)), -1).astype(np.int32)
        last[3] = -1
        eng.set_last_items(last)
        for users in (np.arange(U, dtype=np.int32), np.asarray([5], np.int32), (np.arange(300) % U).astype(np.int32)):
            want = P.predict(*_tables(eng), users[:U], last)[np.arange(len(users)) % min(len(users), U)]
            got = eng.score(users).cpu().numpy()
            assert got.shape == (len(users), I)
            assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), (pairwise, len(users))


def test_an_empty_batch_is_a_no_op():
    """batch == 0: nothing is launched, the loss is two zeros, no table and no step counter moves"""
    import torch
    tabs = _tables0(5, 6, 4, 3, 1)
    eng = _new(tabs, 0.1, 0.01, 0.02, 8, 2, "bpr", True, "adam")
    dev = eng.UI.device
    loss2 = torch.ones(2, device=dev)
    i32 = torch.zeros(0, dtype=torch.int32, device=dev)
    eng.step(i32, torch.zeros((0, 2), dtype=torch.int32, device=dev), i32, i32, loss2)
    assert loss2.cpu().numpy().tolist() == [0.0, 0.0] and eng.t == 0 and eng.adam.t == 0
    assert all(np.array_equal(t, w) for t, w in zip(_tables(eng), tabs)) and _zero_G(eng)


@pytest.mark.parametrize("pairwise", [True, False])
def test_high_order_one_is_fpmc(pairwise):
    """L = 1 (deviation c): alpha = 1, so the row tables follow the restatement over three gd steps; W, b and h move
    by exactly the regulariser — pointwise there is none and they stay bit-equal to their initial values, pairwise W
    and h shrink by (1 - lr reg_w) per step and b stays; score() is FPMC's <UI, IU> + <IL, LI[last]> in float64"""
    import fpmc_restatement as F1
    U, I, d, w, B = 40, 30, 16, 16, 33
    rs = np.random.RandomState(61 + pairwise)
    tabs = _tables0(U, I, d, w, 7, 0.3)
    loss, lr, reg_w = ("bpr" if pairwise else "square"), 0.25, 0.02
    batches = [_random_batch(rs, U, I, B, 1, pairwise) for _ in range(3)]
    eng, st = _against_restatement(tabs, batches, 1, loss, pairwise, lr, reg_w=reg_w)
    W, b, h = _tables(eng)[4:]
    assert np.array_equal(b, tabs[5])
    if pairwise:
        for got, t0 in ((W, tabs[4]), (h, tabs[6])):
            want = t0.astype(np.float64) * (1 - lr * reg_w) ** 3
            assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max()       # three fp32 roundings
    else:
        assert np.array_equal(W, tabs[4]) and np.array_equal(h, tabs[6])
    last = rs.randint(I, size=(U, 1)).astype(np.int32)
    last[9] = -1
    eng.set_last_items(last)
    users = np.arange(U, dtype=np.int32)
    want = F1.predict(*_tables(eng)[:4], users, last[:, 0])
    assert np.abs(eng.score(users).cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("pairwise", [True, False])
def test_permuted_recents(pairwise):
    """x does not depend on the order of the recents: with every instance's recents permuted the loss, the six other
    tables' gradients and score() stay within the bound, and the LI gradient rows are the same rows (each row is the sum
    of its occurrences, wherever they stand)"""
    import torch
    U, I, d, w, B, L = 40, 30, 17, 16, 33, 4
    rs = np.random.RandomState(17)
    tabs = _tables0(U, I, d, w, 9, 0.3)
    users, recents, items, third = _random_batch(rs, U, I, B, L, pairwise)
    perm = np.stack([r[rs.permutation(L)] for r in recents])
    assert (perm != recents).any()
    loss = "bpr" if pairwise else "square"
    out = []
    for rec in (recents, perm):
        eng = _new(tabs, 0.25, 0.01, 0.02, B, L, loss, pairwise)
        loss2 = torch.zeros(2, device=eng.UI.device)
        eng.gradients(*_dev(eng, users, rec, items, third), loss2)
        out.append((float(loss2.cpu().numpy().astype(np.float64).sum()), [eng.G[k].cpu().numpy() for k in P.TABLES]))
    want_loss, want = P.gradients(*(t.astype(np.float64) for t in tabs), users, recents, items, third, pairwise, loss,
                                  0.01, 0.02)
    for got_loss, G in out:
        assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss)
        for name, gr in zip(P.TABLES, G):
            assert np.abs(gr - want[name]).max() <= 1e-5 * np.abs(want[name]).max(), name
    last = rs.randint(I, size=(U, L)).astype(np.int32)
    every = np.arange(U, dtype=np.int32)
    eng.set_last_items(last)
    a = eng.score(every).cpu().numpy()
    eng.set_last_items(np.ascontiguousarray(last[:, ::-1]))
    b = eng.score(every).cpu().numpy()
    want = P.predict(*tabs, every, last)
    assert np.abs(a - want).max() <= 1e-5 * np.abs(want).max() and np.abs(b - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("pairwise", [True, False])
def test_slots_that_take_no_part(pairwise):
    """recents of -1 (and one >= I) mixed into a batch: the restatement with those slots dropped from the softmax and
    from every gradient; an instance whose recents are all absent scores and trains as <UI, IU> alone; an instance
    whose user or item is no table row takes no part at all"""
    U, I, d, w, B, L = 40, 30, 17, 16, 33, 3
    rs = np.random.RandomState(29)
    tabs = _tables0(U, I, d, w, 3, 0.3)
    fed, want = [], []
    for _ in range(2):
        users, recents, items, third = _random_batch(rs, U, I, B, L, pairwise)
        recents[2, 0] = recents[5, 2] = recents[9, 1] = -1
        recents[11] = -1
        f_users, f_rec, f_items = users.copy(), recents.copy(), items.copy()
        f_rec[5, 2] = I                                         # beyond the table: absent as well
        f_users[0], f_items[21], f_users[30] = -1, I, U
        keep = np.setdiff1d(np.arange(B), [0, 21, 30])
        fed.append((f_users, f_rec, f_items, third))
        want.append(tuple(x[keep] for x in (users, recents, items, third)))
    loss = "hinge" if pairwise else "square"                    # sums over the instances, whatever their number
    import torch
    eng = _new(tabs, 0.25, 0.01, 0.02, B, L, loss, pairwise)
    st = P.State(*tabs, learner="gd", lr=0.25)
    loss2 = torch.zeros(2, device=eng.UI.device)
    for k in range(2):
        got = _feed(eng, *fed[k], loss2)
        ref = P.step(st, *want[k], pairwise, loss, 0.01, 0.02)
        assert abs(got - ref) <= 1e-5 * abs(ref), (k, got, ref)
        _close(eng, st, k)
    # the instance without recents alone: x = <UI, IU>, no LI row and no attention weight moves through the loss
    one = (np.asarray([4], np.int32), np.full((1, L), -1, np.int32), np.asarray([6], np.int32),
           np.asarray([8], np.int32) if pairwise else np.asarray([1.0], np.float32))
    eng = _new(tabs, 0.25, 0.0, 0.0, 1, L, loss, pairwise)
    _feed(eng, *one, loss2)
    after = _tables(eng)
    for name, t, t0 in zip(P.TABLES, after, tabs):
        if name in ("UI", "IU"):
            assert (t != t0).any(), name
        else:
            assert np.array_equal(t, t0), name


def test_row_gradients_are_stored_not_added(golden):
    """`gradients` on gradient buffers pre-filled with garbage in the rows the batch looks up: the head of a run STORES
    the row's sum, so the result is bit for bit what clean buffers give; rows the batch did not look up keep what
    they held; the dense buffers are stored whole"""
    import torch
    g = golden
    case = "hinge_gd"
    b = _batch(g, case, 0)
    looked = {"UI": b[0], "IU": np.concatenate([b[2], b[3]]), "IL": np.concatenate([b[2], b[3]]), "LI": b[1].reshape(-1)}
    out = []
    for garbage in (False, True):
        eng = _engine(g, case)
        if garbage:
            for k in P.ROWS:
                eng.G[k][torch.from_numpy(np.unique(looked[k])).long().to(eng.UI.device)] = 1e6
            for k in ("W", "b", "h"):
                eng.G[k].fill_(-7e5)
        loss2 = torch.zeros(2, device=eng.UI.device)
        eng.gradients(*_dev(eng, *b), loss2)
        out.append([eng.G[k].cpu().numpy() for k in P.TABLES])
    for name, clean, dirty in zip(P.TABLES, *out):
        assert np.array_equal(clean, dirty), name
        if name in P.ROWS:
            assert not clean[np.setdiff1d(np.arange(len(clean)), looked[name])].any(), name
    _, want = P.gradients(*P.golden_tables(g, case, "f64", -1), *b, True, "hinge", float(g["reg_mf"]), float(g["reg_w"]))
    for name, got in zip(P.TABLES, out[0]):
        assert np.abs(got - want[name]).max() <= 1e-5 * np.abs(want[name]).max(), name


def test_one_batch_beyond_the_one_workgroup_sort(golden):
    """(5 + L) B = 16,800 keys > 16,384: the sort's segmented multi-workgroup path; L = 3, B = 2100, d = 8, w = 4 on the
    157 x 131 tables, one gd step against the restatement; every other test takes the first path"""
    L, B = 3, 2100
    assert (5 + L) * B > SORT_ONE_WORKGROUP
    U, I = (int(x) for x in golden["shape"])
    rs = np.random.RandomState(2)
    _against_restatement(_tables0(U, I, 8, 4, 6), [_random_batch(rs, U, I, B, L, True)], L, "bpr", True, 0.02)


@pytest.mark.parametrize("learner", ["adam", "momentum"])
def test_two_engines_end_byte_identical(learner):
    """two engines, the same 20 batches: all seven tables and every loss are equal bit for bit"""
    import torch
    U, I, d, w, B, L = 157, 131, 16, 16, 64, 3
    rs = np.random.RandomState(4)
    batches = [_random_batch(rs, U, I, B, L, True) for _ in range(20)]
    tabs = _tables0(U, I, d, w, 12)
    out = []
    for _ in range(2):
        eng = _new(tabs, 0.01, 0.01, 0.02, B, L, "bpr", True, learner)
        loss2 = torch.zeros((20, 2), device=eng.UI.device)
        for k, b in enumerate(batches):
            eng.step(*_dev(eng, *b), loss2[k])
        out.append([getattr(eng, k).clone() for k in P.TABLES] + [loss2.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert (out[0][0].cpu().numpy() != tabs[0]).any()


def test_long_run_against_the_restatement():
    """200 steps of BPR / adam at the shipped shape (d = w = 16, L = 3, B = 64) against the float64 restatement; the
    drift is bounded by that of the SAME restatement run in float32: 4 x its distance from the float64 run + 1e-5
    max|want|, per table and for the last loss.  lr = 0.002; ||h||_1 stays below 80 (asserted), so exp() cannot
    overflow"""
    import torch
    U, I, d, w, B, L, steps, lr = 157, 131, 16, 16, 64, 3, 200, 0.002
    rs = np.random.RandomState(31)
    tabs = _tables0(U, I, d, w, 21, h_ones=True)
    batches = [_random_batch(rs, U, I, B, L, True) for _ in range(steps)]
    eng = _new(tabs, lr, 0.01, 0.02, B, L, "bpr", True, "adam")
    st64 = P.State(*tabs, learner="adam", lr=lr)
    st32 = P.State(*tabs, learner="adam", lr=lr, dtype=np.float32)
    loss2 = torch.zeros((steps, 2), device=eng.UI.device)
    for k, b in enumerate(batches):
        eng.step(*_dev(eng, *b), loss2[k])
        l64 = P.step(st64, *b, True, "bpr", 0.01, 0.02)
        l32 = P.step(st32, *b, True, "bpr", 0.01, 0.02)
    got_loss = float(loss2[-1].cpu().numpy().astype(np.float64).sum())
    print("last loss: device err %.3g, f32 restatement err %.3g" % (abs(got_loss - l64), abs(l32 - l64)))
    assert abs(got_loss - l64) <= 4 * abs(l32 - l64) + 1e-5 * abs(l64)
    for name, t in zip(P.TABLES, _tables(eng)):
        bar = np.abs(st32.var[name].astype(np.float64) - st64.var[name]).max()
        err = np.abs(t.astype(np.float64) - st64.var[name]).max()
        print("%s: device err %.3g, f32 restatement err %.3g" % (name, err, bar))
        assert err <= 4 * bar + 1e-5 * np.abs(st64.var[name]).max(), (name, err, bar)
    assert np.abs(st64.var["h"]).sum() < 80 and np.abs(_tables(eng)[6]).sum() < 80


def test_engine_refusals():
    import torch
    from neurec_amd.fpmcplus import FPMCplusEngine
    z = lambda n, d=4: np.zeros((n, d), np.float32)

    def make(d=4, w=3, L=2, **kw):
        args = dict(loss="bpr", pairwise=True)
        args.update(kw)
        return FPMCplusEngine(z(5, d), z(6, d), z(6, d), z(6, d), z(3 * d, w), z(1, w), z(w, 1), 0.01, 0.0, 0.0, 8, L,
                              **args)
    with pytest.raises(NotImplementedError, match="embedding_size=129 is not supported \\(1 to 128\\)"):
        make(d=129)
    with pytest.raises(NotImplementedError, match="weight_size=65 is not supported \\(1 to 64\\)"):
        make(w=65)
    with pytest.raises(NotImplementedError, match="high_order=17 is not supported \\(1 to 16\\)"):
        make(L=17)
    with pytest.raises(NotImplementedError, match="high_order=0 is not supported \\(1 to 16\\)"):
        make(L=0)
    with pytest.raises(Exception, match="please choose a suitable loss function"):
        make(loss="cross_entropy")                              # not a pairwise loss
    with pytest.raises(Exception, match="please choose a suitable loss function"):
        make(loss="bpr", pairwise=False)
    with pytest.raises(ValueError, match="please select a suitable optimizer"):
        make(learner="lbfgs")
    with pytest.raises(ValueError, match="IU / IL / LI"):
        FPMCplusEngine(z(5), z(6), z(7), z(6), z(12, 3), z(1, 3), z(3, 1), 0.01, 0.0, 0.0, 8, 2)
    with pytest.raises(ValueError, match="W must be \\[3 \\* embedding_size"):
        FPMCplusEngine(z(5), z(6), z(6), z(6), z(8, 3), z(1, 3), z(3, 1), 0.01, 0.0, 0.0, 8, 2)
    with pytest.raises(ValueError, match="b and h"):
        FPMCplusEngine(z(5), z(6), z(6), z(6), z(12, 3), z(1, 3), z(4, 1), 0.01, 0.0, 0.0, 8, 2)
    eng = make()
    dev = eng.UI.device
    i32 = lambda *n: torch.zeros(n, dtype=torch.int32, device=dev)
    loss2 = torch.zeros(2, device=dev)
    with pytest.raises(ValueError, match="max_batch"):
        eng.step(i32(9), i32(9, 2), i32(9), i32(9), loss2)
    with pytest.raises(ValueError, match="recents must be \\[batch, high_order\\]"):
        eng.step(i32(4), i32(4), i32(4), i32(4), loss2)
    with pytest.raises(ValueError, match="recents must be \\[batch, high_order\\]"):
        eng.step(i32(4), i32(2, 4), i32(4), i32(4), loss2)
    with pytest.raises(ValueError, match="same length"):
        eng.step(i32(4), i32(4, 2), i32(3), i32(4), loss2)
    with pytest.raises(ValueError, match="last items"):
        eng.score(np.arange(2, dtype=np.int32))
    with pytest.raises(ValueError, match="last items"):
        eng.set_last_items(np.zeros((5, 3), np.int32))
    assert eng.t == 0 and _zero_G(eng)


# ------------------------------------------------------------------ drop-in
def _run(tmp_path, argv):
    from neurec_amd.main import main
    path = defaults.write_default_configs(str(tmp_path), overrides={
        "data.input.path": os.path.join(str(tmp_path), "dataset"), "data.input.dataset": "toy",
        "test_batch_size": "64", "by_time": "True"}, model_overrides={"FPMCplus": {"learning_rate": "0.01"}})
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return main(argv=argv, properties=path)
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("pairwise", [True, False])
def test_fpmcplus_config_drops_in(tmp_path, pairwise):
    """NeuRec.properties + conf/FPMCplus.properties (the reference's values, at learning_rate 0.01 so that two epochs
    show) + a UIRT file with by_time=True: two epochs through neurec_amd.main in both modes; the reference's log lines
    and the deviations line; the loss finite and lower in epoch 2; the metric columns against the host's metrics on
    engine.score rows fetched by hand (1e-6, the bound test_npe_config_drops_in holds)"""
    from test_fpmc_gpu import _host_metrics, _write_dataset
    from neurec_amd.model.sequential_recommender.FPMCplus import DEVIATIONS
    _write_dataset(str(tmp_path))
    argv = ["--recommender=FPMCplus", "--epochs=2"]
    if not pairwise:
        argv += ["--is_pairwise=False", "--loss_function=cross_entropy"]
    model = _run(tmp_path, argv)
    assert model.engine.pairwise is pairwise and model.engine.L == 3
    folder = os.path.join(str(tmp_path), "log", "toy", "FPMCplus")
    files = os.listdir(folder)
    assert len(files) == 1 and files[0].startswith("toy_FPMCplus_")
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "FPMCplus's hyperparameters:" in text and DEVIATIONS in text
    lines = [ln for ln in text.splitlines()
             if re.search(r"metrics:\t|\[iter \d+ : loss : [0-9.]+, time: [0-9.]+\]|epoch \d+:\t", ln)]
    kinds = [("m" if "metrics:" in ln else "i%s" % re.search(r"iter (\d+)", ln).group(1)
              if "[iter" in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)) for ln in lines]
    assert kinds == ["m", "i1", "e1", "i2", "e2"], kinds
    losses = [float(x) for x in re.findall(r"\[iter \d+ : loss : ([0-9.]+),", text)]
    assert len(losses) == 2 and np.all(np.isfinite(losses)) and losses[1] < losses[0], losses
    evals = re.findall(r"epoch (\d+):\t(.+)", text)
    shown = np.asarray([float(x) for x in evals[-1][1].split()])
    assert np.all(np.isfinite(shown)) and shown.max() > 0
    uni = model.evaluator.evaluator
    users = list(uni.user_pos_test.keys())
    scores = model.engine.score(np.asarray(users, np.int32)).cpu().numpy()
    assert scores.shape == (len(users), model.num_items) and scores.dtype == np.float32
    host = _host_metrics(scores, uni.user_pos_train, uni.user_pos_test, users, uni.top_show, uni.metrics)
    print("metrics: evaluator %s\n         host      %s" % (shown, host))
    assert np.abs(host - shown).max() <= 1e-6
    full = model.predict([0, 5, 9], None).cpu().numpy()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])


def test_refusals(tmp_path, monkeypatch):
    from test_fpmc_gpu import _write_dataset
    _write_dataset(str(tmp_path))
    with pytest.raises(Exception, match="suitable loss function"):
        _run(tmp_path, ["--recommender=FPMCplus", "--epochs=1", "--loss_function=cross_entropy"])   # pairwise mode
    with pytest.raises(ValueError, match="suitable optimizer"):
        _run(tmp_path, ["--recommender=FPMCplus", "--epochs=1", "--learner=lbfgs"])
    with pytest.raises(NotImplementedError, match="1 to 128"):
        _run(tmp_path, ["--recommender=FPMCplus", "--epochs=1", "--embedding_size=129"])
    with pytest.raises(NotImplementedError, match="1 to 64"):
        _run(tmp_path, ["--recommender=FPMCplus", "--epochs=1", "--weight_size=65"])
    with pytest.raises(NotImplementedError, match="1 to 16"):
        _run(tmp_path, ["--recommender=FPMCplus", "--epochs=1", "--high_order=17"])
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)                                # WORLD_SIZE > 1
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(tmp_path, ["--recommender=FPMCplus", "--epochs=1"])
