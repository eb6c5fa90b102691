"""Fossil on the GPU (csrc/fossil.hip through neurec_amd/fossil.py): every step of the reference class's trace,
predict(), the edge shapes and the shapes that can break the fixed-order sums against the float64 restatement, slots
that take no part, determinism, the refusals, the samplers' recents and the drop-in run through neurec_amd.main."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_golden
from neurec_amd import defaults
import fossil_restatement as P
from fossil_restatement import CASES

pytestmark = pytest.mark.gpu

SORT_ONE_WORKGROUP = 16384          # keys nrhip_sort_u64 sorts in one workgroup's LDS (csrc/bpr.hip: kPlanMaxKeys)
MAX_ORDER = 16                      # NRHIP_FOSSIL_MAX_ORDER


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_fossil")


def _engine(g, case, **kw):
    from neurec_amd.fossil import FossilEngine
    loss, learner, pairwise, L, regs, alpha = CASES[case]
    c1, Q, bias, eta, eb = P.initial_tables(g, case)
    return FossilEngine(c1, Q, eta, eb, P.golden_matrix(g), float(g["learning_rate"]), regs, alpha, 64, loss=loss,
                        pairwise=pairwise, learner=learner, bias=bias, **kw)


def _feed(eng, users, recents, items, third, loss2):
    import torch
    dev = eng.c1.device
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    eng.step(t(users, torch.int32), t(recents, torch.int32), t(items, torch.int32),
             t(third, torch.int32 if eng.pairwise else torch.float32), loss2)
    return float(loss2.cpu().numpy().astype(np.float64).sum())


def _tables(eng):
    return [getattr(eng, k).cpu().numpy() for k in P.TABLES]


def _batch(g, case, k):
    return tuple(g["%s_%s" % (case, f)][k] for f in ("users", "recents", "items", "third"))


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """The five tables and the loss after every step against the f64 trace: within 4x the reference's own f32-to-f64
    distance of that step and table (read from the golden) plus 1e-5 max|want| — the bound test_fpmc_gpu.py and
    test_fism_gpu.py hold the same comparison to.  Rows outside <case>_rows_* are bit-equal to their initial value."""
    import torch
    g = golden
    eng = _engine(g, case)
    init = P.initial_tables(g, case)
    loss2 = torch.zeros(2, device=eng.c1.device)
    for k in range(len(g[case + "_users"])):
        loss = _feed(eng, *_batch(g, case, k), loss2)
        want, ref32 = g[case + "_f64_loss"][k], g[case + "_f32_loss"][k]
        print("%s step %d loss: device err %.3g, reference f32 err %.3g" % (case, k + 1, abs(loss - want),
                                                                           abs(ref32 - want)))
        assert abs(loss - want) <= 4 * abs(ref32 - want) + 1e-5 * abs(want)
        for j, (name, got, w64, w32) in enumerate(zip(P.TABLES, _tables(eng), P.golden_tables(g, case, "f64", k),
                                                      P.golden_tables(g, case, "f32", k))):
            bar = np.abs(w32.astype(np.float64) - w64).max()
            err = np.abs(got.astype(np.float64) - w64).max()
            print("%s step %d %s: device err %.3g, reference f32 err %.3g" % (case, k + 1, name, err, bar))
            assert err <= 4 * bar + 1e-5 * np.abs(w64).max(), (case, k, name, err, bar)
            still = np.setdiff1d(np.arange(len(got)), g["%s_rows_%s" % (case, name)])
            assert len(still) or name in ("c1", "eta_bias"), (case, name)
            assert np.array_equal(got[still], init[j][still]), (case, k, name)
    for name in ("Q", "bias", "eta"):                          # the row-applied gradient buffers are zero again
        assert not eng.G[name].any().item(), name


def test_predict_matches_the_reference(golden):
    """full and candidate mode after the trained case `bpr_adagrad` for users with |R_u| > L + 1, = L + 1 and = L
    against the reference's rows; users with |R_u| < L and without train items against the restatement (deviation 3)"""
    import torch
    from neurec_amd.model.general_recommender._common import predict_scores
    g = golden
    case = "bpr_adagrad"
    L, alpha = CASES[case][3], CASES[case][5]
    users, cand = g["predict_users"], g["predict_cand"]
    seqs, R = P.sequences(g), P.golden_matrix(g)
    last = P.last_items(seqs, R.shape[0], L)
    eng = _engine(g, case, last_items=last)
    loss2 = torch.zeros(2, device=eng.c1.device)
    for k in range(len(g[case + "_users"])):
        _feed(eng, *_batch(g, case, k), loss2)
    w64, w32 = g["predict_f64"], g["predict_f32"]
    bound = 4 * np.abs(w32 - w64).max() + 1e-5 * np.abs(w64).max()
    got = eng.score(users).cpu().numpy().astype(np.float64)
    print("predict: device err %.3g, reference f32 err %.3g" % (np.abs(got - w64).max(), np.abs(w32 - w64).max()))
    assert got.shape == w64.shape and np.abs(got - w64).max() <= bound
    Pf, Qf = eng.eval_factors(eng.last_items)
    assert eng.eval_factors(eng.last_items)[0] is Pf         # rebuilt only after a step
    assert Pf.shape == (R.shape[0], 17) and Qf.shape == (R.shape[1], 17)
    full = predict_scores(Pf, Qf, users.tolist(), None)
    assert np.abs(full - w64).max() <= bound
    got_c = predict_scores(Pf, Qf, users.tolist(), [c.tolist() for c in cand])
    c64, c32 = g["predict_cand_f64"], g["predict_cand_f32"]
    assert np.abs(np.stack(got_c) - c64).max() <= 4 * np.abs(c32 - c64).max() + 1e-5 * np.abs(c64).max()
    assert all(np.array_equal(r, full[k][c]) for k, (r, c) in enumerate(zip(got_c, cand)))
    deg = np.diff(R.indptr)
    short = np.asarray([np.flatnonzero(deg == 1)[0], np.flatnonzero(deg == 2)[0], np.flatnonzero(deg == 0)[0]], np.int32)
    tabs = _tables(eng)
    want = P.predict(R, *tabs, short, alpha, last)
    got_s = eng.score(short).cpu().numpy()
    assert np.abs(got_s - want).max() <= 1e-5 * np.abs(want).max()
    assert np.array_equal(got_s[2], tabs[2])                 # no train items: the bias, bit for bit


# ------------------------------------------------------------------ shapes the trace does not hold
def _pattern(U=40, I=50, seed=3, longest=45):
    """a random U x I pattern whose rows hold 0 to `longest` items (the last two items are in no row), and the users'
    sequences: a seeded permutation of the row"""
    rs = np.random.RandomState(seed)
    rows, cols, seqs = [], [], {}
    for u in range(U):
        deg = [0, 1, 2, 3, 4, 17, 18][u] if u < 7 else int(rs.randint(2, longest + 1))
        s = rs.choice(I - 2, deg, replace=False).astype(int).tolist()
        if s:
            seqs[u] = s
        rows += [u] * deg
        cols += s
    R = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(U, I))
    R.sort_indices()
    return R, seqs


def _tables0(U, I, d, L, seed, scale):
    rs = np.random.RandomState(seed)
    return [(scale * rs.randn(I, d)).astype(np.float32), (scale * rs.randn(I, d)).astype(np.float32),
            (0.1 * rs.randn(I)).astype(np.float32), (0.3 * rs.randn(U, L)).astype(np.float32),
            (0.3 * rs.randn(L)).astype(np.float32)]


def _windows(seqs, L):
    return [(u, k) for u, s in seqs.items() for k in range(L, len(s))]


def _batch_of(seqs, I, L, wins, pairwise, rs, neg=None):
    """the batch of the windows `wins` [(user, idx)]: recents seq[idx-1..idx-L]; pairwise: a negative outside the
    sequence; pointwise: label 1 on even slots, label 0 with an item outside the sequence on odd ones"""
    users, recents, items, third = [], [], [], []
    for b, (u, k) in enumerate(wins):
        s = seqs[u]
        out = neg if neg is not None else int(rs.choice(np.setdiff1d(np.arange(I), s)))
        users.append(u)
        recents.append(s[k - L:k][::-1])
        if pairwise:
            items.append(s[k])
            third.append(out)
        else:
            items.append(s[k] if b % 2 == 0 else out)
            third.append(1.0 if b % 2 == 0 else 0.0)
    return (np.asarray(users, np.int32), np.asarray(recents, np.int32).reshape(len(wins), L),
            np.asarray(items, np.int32), np.asarray(third, np.int32 if pairwise else np.float32))


def _against_restatement(R, tabs, batches, pairwise, loss, alpha, lr, regs=(0.01, 0.02, 0.03), learner="gd",
                         max_batch=None, kept=None):
    """the engine and the float64 restatement fed the same batches (`kept`: the restatement's, where they differ): loss
    and the five tables within 1e-5 max|want| after every step (fp32 storage of O(0.1) tables and fp32 loss sums).
    The learner is plain gradient descent with a large step: the update is linear in the gradient, so a wrong or
    missing term of any gradient shows at its full size"""
    import torch
    from neurec_amd.fossil import FossilEngine
    c1, Q, bias, eta, eb = tabs
    eng = FossilEngine(c1, Q, eta, eb, R, lr, regs, alpha, max_batch or max(len(b[0]) for b in batches), loss=loss,
                       pairwise=pairwise, learner=learner, bias=bias)
    st = P.State(*tabs, learner=learner, lr=lr)
    loss2 = torch.zeros(2, device=eng.c1.device)
    for k, b in enumerate(batches):
        got = _feed(eng, *b, loss2)
        want = P.step(st, R, *(kept[k] if kept else b), pairwise, loss, alpha, regs)
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
        for name, t in zip(P.TABLES, _tables(eng)):
            err = np.abs(t - st.var[name]).max()
            assert err <= 1e-5 * np.abs(st.var[name]).max(), (name, k, err)
    return eng, st


LOSSES = [(True, "bpr"), (True, "hinge"), (True, "square"), (False, "cross_entropy"), (False, "square")]


@pytest.mark.parametrize("L", [1, 2, 3, MAX_ORDER])
@pytest.mark.parametrize("d", [1, 16, 20, 64, 65, 128])
def test_edges_against_the_float64_restatement(d, L):
    """every lane layout (d = 1, 16, 20, 64, 65, 128) crossed with high_order 1, 2, 3 and the bound, every loss of both
    modes and alpha in {0, 0.5}: a batch of 33 random windows and a last batch of 1 on a random 40 x 50 pattern whose
    rows hold 0 to 45 items, two gd steps; then every user's scores"""
    R, seqs = _pattern()
    U, I = R.shape
    wins = _windows(seqs, L)
    scale = 0.5 if d == 1 else 0.3 if d <= 20 else 0.1
    for n, (pairwise, loss) in enumerate(LOSSES):
        for alpha in (0.0, 0.5):
            rs = np.random.RandomState(1000 * d + 10 * L + n)
            batches = [_batch_of(seqs, I, L, [wins[k] for k in rs.choice(len(wins), B)], pairwise, rs)
                       for B in (33, 1)]
            eng, st = _against_restatement(R, _tables0(U, I, d, L, d + L, scale), batches, pairwise, loss, alpha,
                                           0.05 if pairwise else 0.1)
    last = P.last_items(seqs, U, L)
    users = np.arange(U, dtype=np.int32)
    want = P.predict(R, *[st.var[k] for k in P.TABLES], users, alpha, last)
    assert np.abs(eng.score(users, last).cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("pairwise", [False, True])
@pytest.mark.parametrize("shape", ["one user", "one target", "recent and target", "empty then one"])
def test_shapes_that_can_break_the_fixed_order_sums(shape, pairwise):
    """one user filling a whole batch of 128 (runs longer than a wavefront; its consecutive windows make one item the
    target of one instance, a recent of others and stand at every eta column); one item as the target of every
    instance (pairwise: as every negative); two consecutive windows alone; B = 0 followed by a final batch of 1"""
    L, d = 3, 20
    R, seqs = _pattern()
    U, I = R.shape
    rs = np.random.RandomState(11)
    wins = _windows(seqs, L)
    longest = max(seqs, key=lambda u: len(seqs[u]))
    own = [(longest, k) for k in range(L, len(seqs[longest]))]
    if shape == "one user":
        batches = [_batch_of(seqs, I, L, [own[k % len(own)] for k in range(128)], pairwise, rs)]
        assert len(set(batches[0][0].tolist())) == 1
        assert P.edge_patterns(*batches[0], pairwise)["two columns"]
    elif shape == "one target":
        b = _batch_of(seqs, I, L, [wins[k] for k in rs.choice(len(wins), 96)], pairwise, rs, neg=I - 1)
        if not pairwise:                                       # every slot: label 0 on the one item
            b = (b[0], b[1], np.full(96, I - 1, np.int32), np.zeros(96, np.float32))
        batches = [b]
        assert len(set((b[3] if pairwise else b[2]).tolist())) == 1
    elif shape == "recent and target":
        batches = [_batch_of(seqs, I, L, own[:2], True, rs)]
        if not pairwise:
            batches = [(batches[0][0], batches[0][1], batches[0][2], np.ones(2, np.float32))]
        assert batches[0][2][0] == batches[0][1][1][0]         # the first target is the second's most recent item
    else:
        empty = _batch_of(seqs, I, L, [], pairwise, rs)
        batches = [empty, _batch_of(seqs, I, L, [own[0]], pairwise, rs)]
        assert len(empty[0]) == 0 and len(batches[1][0]) == 1
    _against_restatement(R, _tables0(U, I, d, L, 7, 0.3), batches, pairwise, "bpr" if pairwise else "square", 0.5,
                         0.02, max_batch=128)


@pytest.mark.parametrize("pairwise", [False, True])
def test_one_batch_beyond_the_one_workgroup_sort(pairwise):
    """The step sorts 2 N keys (N = B pointwise, 2 B pairwise): one workgroup's LDS network up to 16,384 keys, the
    segmented multi-workgroup network beyond.  The smallest batch whose keys exceed it, against the restatement at
    d = 16, L = 2; every other test takes the first path."""
    per = 4 if pairwise else 2
    B = SORT_ONE_WORKGROUP // per + 1
    assert per * (B - 1) <= SORT_ONE_WORKGROUP < per * B
    L = 2
    R, seqs = _pattern(longest=12)
    U, I = R.shape
    rs = np.random.RandomState(2)
    wins = _windows(seqs, L)
    batches = [_batch_of(seqs, I, L, [wins[k] for k in rs.randint(len(wins), size=B)], pairwise, rs, neg=I - 1)]
    _against_restatement(R, _tables0(U, I, 16, L, 6, 0.1), batches, pairwise, "bpr" if pairwise else "square", 0.5,
                         0.0005)


def _bad_slots(R, seqs, L, pairwise, rs):
    """(the batch as fed, the slots that take no part): a user outside the table, a user with |R_u| = L, an item, a
    negative and a recent outside [0, I), and a recent that is a table row but no train item of its user"""
    U, I = R.shape
    wins = _windows(seqs, L)
    users, recents, items, third = _batch_of(seqs, I, L, [wins[k] for k in rs.choice(len(wins), 33)], pairwise, rs)
    users[0], users[7], items[21], items[32], recents[12, 0], recents[13, L - 1] = -1, U, -1, I, I, -1
    u3 = [u for u, s in seqs.items() if len(s) == L][0]       # |R_u| = L: no window
    users[3], recents[3], items[3] = u3, seqs[u3][::-1], seqs[u3][0]
    recents[17, 1] = I - 2                                     # in no train row
    other = [h for h in range(I - 2) if h not in seqs[int(users[25])]][0]
    recents[25, 0] = other                                     # a train item of other users only
    out = [0, 7, 21, 32, 12, 13, 3, 17, 25]
    if pairwise:
        third[5], third[30] = I, -1
        out += [5, 30]
    return (users, recents, items, third), out


@pytest.mark.parametrize("pairwise", [False, True])
def test_slots_that_take_no_part(pairwise):
    """A slot (a whole pair) with a user, item, negative or recent that is no table row, a user with |R_u| <= L, or a
    recent that is not in its user's train row takes no part: two gd steps give the loss and tables of the restatement
    fed the same batches without those slots.  And they leave every table, gradient buffer, row flag and optimiser
    state untouched: under each of the five learners an engine fed the batches with those slots ends bit-identical to
    one fed the batches without them (the sums run in batch order, which dropping slots keeps)."""
    import torch
    from neurec_amd.fossil import FossilEngine
    L, d = 3, 16
    R, seqs = _pattern()
    U, I = R.shape
    rs = np.random.RandomState(29)
    fed, kept = [], []
    for _ in range(2):
        b, out = _bad_slots(R, seqs, L, pairwise, rs)
        keep = np.setdiff1d(np.arange(33), out)
        fed.append(b)
        kept.append(tuple(x[keep] for x in b))
        assert len(P.instances(R, L, *b, pairwise)) == len(keep) * (2 if pairwise else 1)
    loss, lr = ("bpr", 0.05) if pairwise else ("square", 0.1)
    _against_restatement(R, _tables0(U, I, d, L, 3, 0.3), fed, pairwise, loss, 0.5, lr, kept=kept)
    for learner in ("adam", "gd", "adagrad", "rmsprop", "momentum"):
        ends = []
        for batches in (fed, kept):
            tabs = _tables0(U, I, d, L, 3, 0.3)
            eng = FossilEngine(tabs[0], tabs[1], tabs[3], tabs[4], R, 0.05, (0.01, 0.02, 0.03), 0.5, 33, loss=loss,
                               pairwise=pairwise, learner=learner, bias=tabs[2])
            loss2 = torch.zeros(2, device=eng.c1.device)
            for b in batches:
                _feed(eng, *b, loss2)
            names = P.TABLES
            ends.append([getattr(eng, k) for k in names] + [eng.G[k] for k in names] +
                        [s[k] for s in (eng.s0, eng.s1) for k in names if s[k] is not None] +
                        [f for f in (eng.flag_Q, eng.flag_bias, eng.flag_eta) if f is not None])
        assert len(ends[0]) == len(ends[1]) and all(torch.equal(x, y) for x, y in zip(*ends)), learner


@pytest.mark.parametrize("case", ["bpr_adagrad", "ce_adam", "square_momentum"])
def test_two_engines_end_byte_identical(golden, case):
    """the same three batches twice (the first batch again as the third); a row-optimiser learner among the cases"""
    import torch
    g = golden
    out = []
    for _ in range(2):
        eng = _engine(g, case)
        loss2 = torch.zeros(2, device=eng.c1.device)
        n = len(g[case + "_users"])
        losses = [_feed(eng, *_batch(g, case, k % n), loss2) for k in range(3)]
        out.append([getattr(eng, k).clone() for k in P.TABLES] + [losses])
    assert all(torch.equal(a, b) for a, b in zip(out[0][:5], out[1][:5])) and out[0][5] == out[1][5]


def test_engine_refusals():
    """d = 0, d = 129, L = 0, L above the bound, an unknown loss, an unknown learner: refused when the engine is built,
    before anything is launched; a batch larger than max_batch: refused by step(); the C entry names the bound"""
    import torch
    from neurec_amd._lib import FossilStepArgs, call
    from neurec_amd.fossil import FossilEngine
    R, _ = _pattern()
    U, I = R.shape
    z = lambda n, d: np.zeros((n, d), np.float32)
    mk = lambda d=4, L=3, **kw: FossilEngine(z(I, d), z(I, d), z(U, L), z(1, L), R, 0.01, [0, 0, 0], 0.5, 8, **kw)
    for d in (0, 129):
        with pytest.raises(NotImplementedError, match="1 to 128"):
            mk(d=d)
    for L in (0, MAX_ORDER + 1):
        with pytest.raises(NotImplementedError, match="1 to %d" % MAX_ORDER):
            mk(L=L)
    with pytest.raises(Exception, match="please choose a suitable loss function"):
        mk(loss="hinge", pairwise=False)
    with pytest.raises(Exception, match="please choose a suitable loss function"):
        mk(loss="cross_entropy", pairwise=True)
    with pytest.raises(ValueError, match="please select a suitable optimizer"):
        mk(learner="lbfgs")
    eng = mk()
    dev = eng.c1.device
    i32 = torch.zeros(9, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="max_batch"):
        eng.step(i32, torch.zeros((9, 3), dtype=torch.int32, device=dev), i32, i32, torch.zeros(2, device=dev))
    with pytest.raises(ValueError, match="high_order"):
        eng.step(i32[:4], torch.zeros((4, 2), dtype=torch.int32, device=dev), i32[:4], i32[:4],
                 torch.zeros(2, device=dev))
    for field, value, text in (("L", MAX_ORDER + 1, "high_order 17 outside 1..16"),
                               ("d", 129, "embedding_size 129 outside 1..128")):
        a = FossilStepArgs()
        a.d, a.L = 4, 3
        setattr(a, field, value)
        with pytest.raises(NotImplementedError, match=text):
            call("nrhip_fossil_step", C.byref(a), None)
    assert eng.t == 0 and not eng.G["c1"].any().item()


# ------------------------------------------------------------------ the samplers' recents
SEQS = {0: [3, 1, 4, 11, 5, 9], 1: [9, 2], 2: [6], 3: [5, 3, 8, 0, 7, 10, 2], 5: [2, 11, 1, 4]}


class _ToyTimed:
    num_users, num_items = 6, 12

    def get_user_train_dict(self, by_time=False):
        return {u: (list(s) if by_time else sorted(s)) for u, s in SEQS.items()}


@pytest.mark.parametrize("pairwise", [False, True])
def test_time_order_samplers_at_high_order_3(pairwise):
    """one epoch of each time-order sampler at high_order = 3 with as_tensors=True: through `recents_for_engine` the
    recents are seq[idx-1], seq[idx-2], seq[idx-3]; label-0 slots carry a window's recents; every window comes once"""
    from neurec_amd.data import TimeOrderPairwiseSampler, TimeOrderPointwiseSampler
    from neurec_amd.model.sequential_recommender.Fossil import recents_for_engine
    L = 3
    if pairwise:
        it = TimeOrderPairwiseSampler(_ToyTimed(), high_order=L, neg_num=1, batch_size=4, shuffle=True, as_tensors=True)
    else:
        it = TimeOrderPointwiseSampler(_ToyTimed(), high_order=L, neg_num=2, batch_size=4, shuffle=True,
                                       as_tensors=True)
    n_windows = sum(max(len(s) - L, 0) for s in SEQS.values())
    assert it.stream.n_slots == (n_windows if pairwise else 3 * n_windows)
    seen = []
    for users, recent, items, third in it:
        rec = recents_for_engine(recent, L)
        assert rec.is_contiguous() and tuple(rec.shape) == (users.numel(), L)
        u, r, i, t = (x.cpu().numpy() for x in (users, rec, items, third))
        for b in range(len(u)):
            s = SEQS[int(u[b])]
            if pairwise or t[b] == 1.0:
                k = s.index(int(i[b]))
                assert k >= L and r[b].tolist() == [s[k - 1], s[k - 2], s[k - 3]]
                seen.append((int(u[b]), k))
            else:
                assert int(i[b]) not in s
                assert any(r[b].tolist() == [s[k - 1], s[k - 2], s[k - 3]] for k in range(L, len(s)))
    assert sorted(seen) == sorted((u, k) for u, s in SEQS.items() for k in range(L, len(s)))


# ------------------------------------------------------------------ drop-in
FOSSIL_PROPERTIES = """[hyperparameters]
epochs=100
batch_size=256
embedding_size=16
regs=[0.00,0.00,0.0]
alpha=0.5
learning_rate=0.001
learner=adagrad
is_pairwise=True
high_order=3
num_neg=4
loss_function=bpr
init_method=uniform
stddev=0.01
verbose=1
"""


def _run(tmp_path, argv):
    from neurec_amd.main import main
    path = defaults.write_default_configs(str(tmp_path), overrides={
        "data.input.path": os.path.join(str(tmp_path), "dataset"), "data.input.dataset": "toy",
        "test_batch_size": "64", "by_time": "True"})
    with open(os.path.join(str(tmp_path), "conf", "Fossil.properties"), "w") as f:
        f.write(FOSSIL_PROPERTIES)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return main(argv=argv, properties=path)
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("pairwise", [True, False])
def test_fossil_config_drops_in(tmp_path, monkeypatch, pairwise):
    """NeuRec.properties + the reference's conf/Fossil.properties + a UIRT file with by_time=True: two epochs through
    neurec_amd.main in both modes; the reference's log lines and the deviation line; the epoch-1 loss against the
    restatement on the same stream, over the number of instances; the evaluation through the factor path, its metrics
    against the host's on engine.score (1e-6, the bound test_fpmc_config_drops_in holds)"""
    from test_fpmc_gpu import _host_metrics, _write_dataset
    from neurec_amd.data import TimeOrderPairwiseSampler, TimeOrderPointwiseSampler
    from neurec_amd.model.sequential_recommender.Fossil import STRUCTURE, recents_for_engine
    from neurec_amd.util.tool import get_initializer
    _write_dataset(str(tmp_path))
    argv = ["--recommender=Fossil", "--epochs=2"] + \
        ([] if pairwise else ["--is_pairwise=False", "--loss_function=cross_entropy"])
    model = _run(tmp_path, argv)
    folder = os.path.join(str(tmp_path), "log", "toy", "Fossil")
    files = os.listdir(folder)
    assert len(files) == 1 and files[0].startswith("toy_Fossil_")
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "Fossil's hyperparameters:" in text and STRUCTURE in text
    lines = [ln for ln in text.splitlines()
             if re.search(r"metrics:\t|\[iter \d+ : loss : [0-9.]+, time: [0-9.]+\]|epoch \d+:\t", ln)]
    kinds = [("m" if "metrics:" in ln else "i%s" % re.search(r"iter (\d+)", ln).group(1)
              if "[iter" in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)) for ln in lines]
    assert kinds == ["m", "i1", "e1", "i2", "e2"], kinds
    evals = re.findall(r"epoch (\d+):\t(.+)", text)
    shown = np.asarray([float(x) for x in evals[-1][1].split()])
    assert np.all(np.isfinite(shown)) and shown.max() > 0

    # the epoch-1 loss: the same stream (the sampler's epoch 0) through the restatement, over the number of instances
    ds = model.dataset
    L, d = 3, 16
    if pairwise:
        it = TimeOrderPairwiseSampler(ds, high_order=L, neg_num=1, batch_size=256, shuffle=True, as_tensors=True)
    else:
        it = TimeOrderPointwiseSampler(ds, high_order=L, neg_num=4, batch_size=256, shuffle=True, as_tensors=True)
    seqs = ds.get_user_train_dict(by_time=True)
    n_windows = sum(max(len(s) - L, 0) for s in seqs.values())
    assert it.stream.n_slots == (n_windows if pairwise else 5 * n_windows)
    init = get_initializer("uniform", 0.01, seed=2017)
    c1, Q = init([ds.num_items, d]), init([ds.num_items, d])
    eta, eb = init([ds.num_users, L]), init([1, L])
    st = P.State(c1, Q, None, eta, eb, learner="adagrad", lr=0.001)
    R = sp.csr_matrix(ds.train_matrix)
    R.sort_indices()
    total = 0.0
    for users, recent, items, third in it:
        total += P.step(st, R, users.cpu().numpy(), recents_for_engine(recent, L).cpu().numpy(), items.cpu().numpy(),
                        third.cpu().numpy(), pairwise, "bpr" if pairwise else "cross_entropy", 0.5, (0.0, 0.0, 0.0))
    logged = float(re.search(r"\[iter 1 : loss : ([0-9.]+),", text).group(1))
    want = total / it.stream.n_slots
    print("epoch-1 loss: logged %.6f, restatement %.9f" % (logged, want))
    assert abs(logged - want) <= 1e-4 * abs(want) + 5e-7                  # %f prints six decimals

    # the evaluator took the factor path (predict is never called), and its metrics are the host's on engine.score
    uni = model.evaluator.evaluator
    monkeypatch.setattr(model, "predict", lambda *a, **k: (_ for _ in ()).throw(AssertionError("predict called")))
    again = np.asarray([float(x) for x in model.evaluator.evaluate(model).split()])
    assert np.array_equal(again, shown)
    monkeypatch.undo()
    users = list(uni.user_pos_test.keys())
    scores = model.engine.score(np.asarray(users, np.int32)).cpu().numpy()
    host = _host_metrics(scores, uni.user_pos_train, uni.user_pos_test, users, uni.top_show, uni.metrics)
    print("metrics: evaluator %s\n         host      %s" % (shown, host))
    assert np.abs(host - shown).max() <= 1e-6
    full = model.predict([0, 5, 9], None)
    assert full.shape == (3, model.num_items) and full.dtype == np.float32
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])


def test_refusals(tmp_path, monkeypatch):
    from test_fpmc_gpu import _write_dataset
    _write_dataset(str(tmp_path))
    with pytest.raises(Exception, match="suitable loss function"):
        _run(tmp_path, ["--recommender=Fossil", "--epochs=1", "--loss_function=cross_entropy"])   # not a pairwise loss
    with pytest.raises(ValueError, match="suitable optimizer"):
        _run(tmp_path, ["--recommender=Fossil", "--epochs=1", "--learner=lbfgs"])
    with pytest.raises(NotImplementedError, match="128"):
        _run(tmp_path, ["--recommender=Fossil", "--epochs=1", "--embedding_size=129"])
    with pytest.raises(NotImplementedError, match="1 to 16"):
        _run(tmp_path, ["--recommender=Fossil", "--epochs=1", "--high_order=17"])
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)                                # WORLD_SIZE > 1
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(tmp_path, ["--recommender=Fossil", "--epochs=1"])
