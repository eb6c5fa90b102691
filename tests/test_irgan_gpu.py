"""IRGAN on the GPU (csrc/irgan.hip through neurec_amd/irgan.py): the reference class's recorded runs replayed through
d_step and its recorded samples (tests/golden/tfgraph_irgan.npz) — every table after every step, the ratings in both
modes; the integer weights against the float64 restatement; the draws against the restatement's, bit for bit, given the
weights the device reports; the D data's layout; both steps on the edge shapes against the float64 restatement, which
test_irgan_cpu.py holds to the same trace and to autograd; determinism, empty work, and the drop-in run through
neurec_amd.main in a child process.

The tolerance is the project's rule (`_close` of test_gru4rec_gpu.py): 4 x the float32 reference's own distance from the
float64 one for that tensor and step, plus 1e-5 max|want|.  For the trace the distance is the reference's, read from the
golden; on the edge shapes it is the restatement's float32 run's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import irgan_restatement as P
from test_irgan_cpu import recorded_steps, wanted
from test_gru4rec_gpu import _close

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "tfgraph_irgan.npz"))


def _engine(tables, M, lr=P.LR, g_reg=0.0, d_reg=0.1 / 16, d_tau=0.2, batch=P.BATCH, seed=2018):
    from neurec_amd.irgan import IRGANEngine
    return IRGANEngine(tables, M, lr, g_reg, d_reg, d_tau, batch, seed=seed)


def _matrix(g):
    return sp.csr_matrix((np.ones(len(g["indices"]), np.float32), g["indices"], g["indptr"]), shape=tuple(g["shape"]))


def _golden_engine(g, case):
    g_reg, d_reg, d_tau = P.CASES[case][:3]
    U, I = (int(x) for x in g["shape"])
    init = P.init_tables(U, I, P.FACTORS, int(g["%s_init_seed" % case]))
    return _engine(init, _matrix(g), g_reg=g_reg, d_reg=d_reg, d_tau=d_tau), init


# ------------------------------------------------------------------ the reference's trace
@pytest.mark.parametrize("case", sorted(P.CASES))
def test_steps_match_the_reference_trace(golden, case):
    """The recorded run replayed through d_step and g_step(user, samples): every table of the stepped network after
    every step of the first epoch, and all six after the last step of the second, against the float64 trace under the
    trace's own f32-to-f64 distance; a D step leaves G's tables bit-unchanged and a G step D's; then the ratings for
    every user and for candidates under the distance of the reference's own float32 ratings."""
    g = golden
    eng, init = _golden_engine(g, case)
    kinds = str(g["%s_kinds" % case])
    S1, n = len(kinds) // 2, {"d": 0, "g": 0}
    before = eng.tables()
    for s, (kind, args) in enumerate(recorded_steps(g, case)):
        (eng.d_step if kind == "d" else eng.g_step)(*args)
        now = eng.tables()
        for k in P.NAMES:
            if k[0] != kind:
                assert np.array_equal(now[k], before[k]), (case, s, kind, k)
            elif s < S1:
                _close(now[k], wanted(g, case, init, k, n[kind]), float(g["%s_gap_%s" % (case, k)][n[kind]]),
                       "%s step %d %s" % (case, s, k))
        n[kind] += 1
        before = now
    for k in P.NAMES:
        _close(before[k], init[k].astype(np.float64) + g["%s_end_%s" % (case, k)], float(g["%s_endgap_%s" % (case, k)]),
               "%s end %s" % (case, k))
    w64, w32 = g["%s_ratings_f64" % case], g["%s_ratings_f32" % case].astype(np.float64)
    bar = np.abs(w32 - w64).max()
    got = eng.score(np.arange(23)).cpu().numpy()
    assert got.shape == (23, 67)
    _close(got, w64, bar, "%s ratings" % case)
    some = np.asarray([22, 0, 4, 4, 11])
    _close(eng.score(some).cpu().numpy(), w64[some], bar, "%s ratings of some users" % case)
    sizes = np.asarray([3, 0, 1, 7, 2])
    items = np.random.RandomState(5).randint(0, 67, int(sizes.sum()))
    want = np.concatenate([w64[u][items[a:a + m]] for u, a, m in zip(some, np.cumsum(sizes) - sizes, sizes)])
    _close(eng.forward(some, items, sizes).cpu().numpy(), want, bar, "%s candidates" % case)
    assert eng.score(np.zeros(0, np.int32)).shape == (0, 67) and eng.forward([], [], []).numel() == 0


def test_a_d_pass_is_its_steps(golden):
    """d_pass(order, data) in one call equals the recorded batches stepped one by one, bit for bit, the short last batch
    included; its loss terms are the restatement's"""
    import torch
    g, case = golden, "defaults"
    one, init = _golden_engine(g, case)
    two, _ = _golden_engine(g, case)
    lo, hi = (int(x) for x in g["%s_pass_ptr" % case][:2])
    triples = tuple(g["%s_pass_%s" % (case, k)][lo:hi] for k in ("users", "items", "labels"))
    order = g["%s_pass_order" % case][lo:hi]
    steps = -(-(hi - lo) // P.BATCH)
    assert (hi - lo) % P.BATCH != 0
    loss = torch.zeros((steps, 3), device=one.dev)
    data = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(one.dev) for x in triples)
    one.d_pass(order, loss, data=data)
    r64 = P.IRGAN(init, g["indptr"], g["indices"], P.LR, *P.CASES[case][:2])
    r32 = P.IRGAN(init, g["indptr"], g["indices"], P.LR, *P.CASES[case][:2], dtype=np.float32)
    each = torch.zeros(3, device=two.dev)
    for s in range(steps):
        idx = order[s * P.BATCH:(s + 1) * P.BATCH]
        batch = tuple(x[idx] for x in triples)
        two.d_step(*batch, loss_out=each)
        assert np.array_equal(each.cpu().numpy(), loss[s].cpu().numpy())
        t64, t32 = np.asarray(r64.d_step(*batch), np.float64), np.asarray(r32.d_step(*batch), np.float64)
        _close(loss[s].cpu().numpy(), t64, np.abs(t32 - t64).max(), "loss terms of step %d" % s)
    a, b = one.tables(), two.tables()
    assert all(np.array_equal(a[k], b[k]) for k in P.NAMES)


# ------------------------------------------------------------------ weights and draws
def _logit_rows(I):
    """rows of logits [4, I]: random, random and steep, all equal, one 200 above the rest"""
    rs = np.random.RandomState(I)
    z = np.stack([rs.uniform(-1, 1, I), rs.uniform(-6, 6, I), np.full(I, 0.37), rs.uniform(-1, 1, I)]).astype(np.float32)
    z[3, I // 2] += 200.0
    return z


@pytest.fixture(scope="module")
def tiny_engine():
    M = sp.csr_matrix(np.eye(3, 5, dtype=np.float32))
    return _engine(P.init_tables(3, 5, 2, 1), M)


@pytest.mark.parametrize("tau", [0.2, 1.0])
@pytest.mark.parametrize("I", [1, 2, 63, 64, 65, 4099])
def test_the_weights_match_the_float64_restatement(tiny_engine, I, tau):
    """w / 2^31 against the float64 restatement under 4 x the float32 restatement's own distance plus 2^-31; the largest
    logit's weight is 2^31 exactly, equal logits give equal weights, and a logit 200 above the rest leaves one weight"""
    z = _logit_rows(I)
    got = tiny_engine.weights_of(z, tau)
    assert got.shape == (4, I) and got.dtype == np.uint32
    for r in range(4):
        w64, w32 = P.weights(z[r], tau), P.weights(z[r], tau, np.float32)
        bar = np.abs(w32.astype(np.float64) - w64.astype(np.float64)).max() / 2.0 ** 31
        err = np.abs(got[r].astype(np.float64) - w64.astype(np.float64)).max() / 2.0 ** 31
        print("I=%d tau=%g row %d: device err %.3g, float32 restatement err %.3g" % (I, tau, r, err, bar))
        assert err <= 4 * bar + 2.0 ** -31, (I, tau, r, err, bar)
        assert got[r].max() == 2 ** 31 and got[r][np.argmax(z[r])] == 2 ** 31
    assert (got[2] == 2 ** 31).all()
    assert np.count_nonzero(got[3]) == 1 and got[3][I // 2] == 2 ** 31


@pytest.mark.parametrize("I", [1, 2, 63, 64, 65, 4099])
def test_the_draws_are_the_restatement_s_bit_for_bit(tiny_engine, I):
    """given the weights the device reports: plain and mixture draws at several users and pass counters; weights whose
    only non-zero entries are the first and the last item; a single non-zero weight, which is always drawn; deg 1; a
    user whose positives include item 0"""
    eng = tiny_engine
    w = eng.weights_of(_logit_rows(I), 0.2)
    rows = [w[0], w[1], w[2], w[3]]
    ends = np.zeros(I, np.uint32)
    ends[0], ends[-1] = 3, 2 ** 31
    rows.append(ends)
    rs = np.random.RandomState(I + 1)
    pos_lists = [np.asarray([0]), np.asarray([I - 1]), np.unique(rs.randint(0, I, 9)), np.unique(np.r_[0, rs.randint(0, I, 40)])]
    for k, wr in enumerate(rows):
        for pos in pos_lists:
            for user, pas in ((0, 0), (7, 3), (29857, 2 ** 33 + 5)):
                got0 = eng.draws(wr, user, pos, 0, pas)
                assert np.array_equal(got0, P.plain_draws(wr, len(pos), eng.seed, pas, user)), (I, k, user, pas)
                got1 = eng.draws(wr, user, pos, 1, pas)
                assert np.array_equal(got1, P.mixture_draws(wr, pos, eng.seed, pas, user)), (I, k, user, pas)
                assert len(got0) == len(pos) and len(got1) == 2 * len(pos)
                assert (wr[got0] > 0).all() and all(wr[i] > 0 or i in pos for i in got1)
        if k == 3:
            assert (eng.draws(wr, 5, np.arange(min(I, 50)), 0, 1) == I // 2).all()       # the single weight, always
    both = eng.draws(ends, 3, np.arange(min(I, 64)), 0, 9)
    assert set(both.tolist()) <= {0, I - 1}
    a, b = eng.draws(rows[1], 3, pos_lists[3], 1, 4), eng.draws(rows[1], 3, pos_lists[3], 1, 5)
    assert I < 3 or not np.array_equal(a, b)                                          # another pass counter, other draws


def test_the_d_data_layout_and_the_skipped_users(golden):
    """offsets and interleaving, the users the any() rule skips absent, the negatives the restatement's given the
    device's weights, reruns bit-identical and a new pass counter new draws"""
    g = golden
    eng, init = _golden_engine(g, "defaults")
    indptr, indices = g["indptr"], g["indices"]
    train = P.train_users(indptr, indices)
    assert eng.train_users.tolist() == train and eng.d_pass_size() == 2 * sum(indptr[u + 1] - indptr[u] for u in train)
    u, i, y = (t.cpu().numpy() for t in eng.d_data())
    assert eng.d_passes == 1 and len(u) == eng.d_pass_size()
    assert u[0::2].tolist() == u[1::2].tolist() == [w for w in train for _ in range(indptr[w + 1] - indptr[w])]
    assert 4 not in u and 9 not in u
    assert i[0::2].tolist() == [int(j) for w in train for j in indices[indptr[w]:indptr[w + 1]]]
    assert (y[0::2] == 1).all() and (y[1::2] == 0).all() and i.min() >= 0 and i.max() < 67
    at = 0
    for w in train:
        deg = int(indptr[w + 1] - indptr[w])
        weights = eng.weights(w, 0.2)
        assert np.array_equal(i[at + 1:at + 2 * deg:2], P.plain_draws(weights, deg, eng.seed, 0, w)), w
        at += 2 * deg
    again, _ = _golden_engine(g, "defaults")
    u2, i2, y2 = (t.cpu().numpy() for t in again.d_data())
    assert np.array_equal(i, i2) and np.array_equal(u, u2) and np.array_equal(y, y2)
    _, i3, _ = (t.cpu().numpy() for t in again.d_data())                                # pass counter 1
    assert not np.array_equal(i, i3) and np.array_equal(i[0::2], i3[0::2])
    part = [t.cpu().numpy() for t in again.d_data(users=[13, 2])]
    assert part[0].tolist() == [13, 13] + [2] * (2 * int(indptr[3] - indptr[2]))


def test_a_g_step_draws_what_the_restatement_draws(golden):
    """a made G step: its samples are the restatement's mixture draws from the weights it reports, its rewards and its
    update the restatement's at those samples; a rerun is bit-identical, another pass counter draws anew"""
    g = golden
    eng, init = _golden_engine(g, "greg")
    g_reg, d_reg = P.CASES["greg"][:2]
    r64 = P.IRGAN(init, g["indptr"], g["indices"], P.LR, g_reg, d_reg)
    r32 = P.IRGAN(init, g["indptr"], g["indices"], P.LR, g_reg, d_reg, dtype=np.float32)
    seen = []
    for user in (2, 11, 13):
        eng.g_step(user)
        items, r = eng.last_draws()
        w = eng.last_weights()
        assert np.array_equal(items, P.mixture_draws(w, r64.pos(user), eng.seed, 0, user)), user
        z = r64.T["g_Q"] @ r64.T["g_P"][user] + r64.T["g_b"]
        w64, w32 = P.weights(z, 1.0), P.weights(z, 1.0, np.float32)
        bar = np.abs(w32.astype(np.float64) - w64.astype(np.float64)).max() / 2.0 ** 31
        assert np.abs(w.astype(np.float64) - w64.astype(np.float64)).max() / 2.0 ** 31 <= 4 * bar + 2.0 ** -31
        (_, want), (_, twin) = r64.rewards(user, items), r32.rewards(user, items)
        _close(r, want, np.abs(twin - want).max(), "rewards of user %d" % user)
        r64.g_step(user, items)
        r32.g_step(user, items)
        now = eng.tables()
        for k in ("g_P", "g_Q", "g_b"):
            _close(now[k], r64.T[k], np.abs(r32.T[k].astype(np.float64) - r64.T[k]).max(), "user %d %s" % (user, k))
        seen.append(items)
    again, _ = _golden_engine(g, "greg")
    for user in (2, 11, 13):
        again.g_step(user)
    a, b = eng.tables(), again.tables()
    assert all(np.array_equal(a[k], b[k]) for k in P.NAMES)
    again.g_passes = 1
    again.g_step(11)
    assert not np.array_equal(again.last_draws()[0], seen[1])


def test_a_g_pass_is_its_user_steps(golden):
    """g_pass() in one call equals g_step over the train users in ascending id, bit for bit; D is only read"""
    g = golden
    one, _ = _golden_engine(g, "steps")
    two, _ = _golden_engine(g, "steps")
    one.g_pass()
    for u in two.train_users:
        two.g_step(int(u))
    a, b = one.tables(), two.tables()
    assert all(np.array_equal(a[k], b[k]) for k in P.NAMES) and one.g_passes == 1 and two.g_passes == 0
    init = P.init_tables(23, 67, P.FACTORS, int(g["steps_init_seed"]))
    assert all(np.array_equal(a[k], init[k]) for k in ("d_P", "d_Q", "d_b"))
    assert not np.array_equal(a["g_Q"], init["g_Q"]) and np.isfinite(a["g_Q"]).all()
    assert np.array_equal(a["g_P"][[4, 9]], init["g_P"][[4, 9]])                        # the skipped users' rows


# ------------------------------------------------------------------ the steps on the edge shapes
N_U, N_I = 6, 1100


def _edge(d):
    rs = np.random.RandomState(100 + d)
    dense = np.zeros((N_U, N_I), np.float32)
    dense[0, [0, 3, 700]] = 1                                       # positives that include item 0
    dense[1, 1099] = 1                                              # deg 1: S = 2
    dense[2, rs.choice(N_I, 40, replace=False)] = 1
    dense[3, [5, 6]] = 1
    tables = P.init_tables(N_U, N_I, d, 50 + d)
    tables["d_b"] = rs.uniform(-0.2, 0.2, N_I).astype(np.float32)
    for k in ("d_P", "d_Q"):
        tables[k] = (tables[k] * 8).astype(np.float32)
    M = sp.csr_matrix(dense)
    M.sort_indices()
    return M, tables


def _pair(M, tables, g_reg, d_reg):
    return tuple(P.IRGAN(tables, M.indptr, M.indices, 0.05, g_reg, d_reg, dt) for dt in (np.float64, np.float32))


D_EDGES = {
    "one_pair": ([2], [17], [1.0]),
    "one_pair_three_times": ([1, 1, 1], [900, 900, 900], [1.0, 0.0, 1.0]),
    "one_user": ([4, 4, 4, 4, 4], [0, 1099, 3, 3, 512], [1.0, 0.0, 0.0, 1.0, 0.0]),
    "mixed_repeats": ([0, 5, 0, 2, 5, 5, 3], [7, 7, 8, 7, 1024, 7, 256], [1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0]),
}


@pytest.mark.parametrize("d", [1, 20, 33, 128])
@pytest.mark.parametrize("name", sorted(D_EDGES))
def test_d_steps_on_the_edge_shapes_match_the_restatement(name, d):
    users, items, labels = D_EDGES[name]
    M, tables = _edge(d)
    eng = _engine(tables, M, lr=0.05, g_reg=0.0, d_reg=0.02)
    r64, r32 = _pair(M, tables, 0.0, 0.02)
    for r in (r64, r32):
        r.d_step(users, items, labels)
    eng.d_step(users, items, labels)
    now = eng.tables()
    for k in ("d_P", "d_Q", "d_b"):
        _close(now[k], r64.T[k], np.abs(r32.T[k].astype(np.float64) - r64.T[k]).max(), "%s d=%d %s" % (name, d, k))
        touched = np.zeros(len(now[k]), bool)
        touched[users if k == "d_P" else items] = True
        assert np.array_equal(now[k][~touched], tables[k][~touched])               # the touched rows only
    assert all(np.array_equal(now[k], tables[k]) for k in ("g_P", "g_Q", "g_b"))


@pytest.mark.parametrize("d", [1, 20, 33, 128])
def test_the_short_last_batch_uses_its_own_size(d):
    """seven triples in batches of three: the regulariser counts 3, 3 and 1 times"""
    import torch
    users, items, labels = D_EDGES["mixed_repeats"]
    M, tables = _edge(d)
    eng = _engine(tables, M, lr=0.05, g_reg=0.0, d_reg=0.02, batch=3)
    r64, r32 = _pair(M, tables, 0.0, 0.02)
    order = np.asarray([6, 0, 3, 2, 5, 1, 4], np.int32)
    data = tuple(torch.from_numpy(np.asarray(x, dt)).to(eng.dev) for x, dt in ((users, np.int32), (items, np.int32),
                                                                                (labels, np.float32)))
    eng.d_pass(order, data=data)
    for s in range(0, 7, 3):
        idx = order[s:s + 3]
        for r in (r64, r32):
            r.d_step(np.asarray(users)[idx], np.asarray(items)[idx], np.asarray(labels)[idx])
    now = eng.tables()
    for k in ("d_P", "d_Q", "d_b"):
        _close(now[k], r64.T[k], np.abs(r32.T[k].astype(np.float64) - r64.T[k]).max(), "short batch d=%d %s" % (d, k))


G_EDGES = {
    # name: (user, samples, g_reg)
    "all_one_item": (2, [77] * 80, 0.0),
    "all_positives": (0, [0, 3, 700, 0, 700, 3], 0.0),
    "two_samples": (1, [1099, 4], 0.0),
    "reg_with_repeats": (3, [5, 900, 900, 5], 0.03),
}


@pytest.mark.parametrize("d", [1, 20, 33, 128])
@pytest.mark.parametrize("name", sorted(G_EDGES))
def test_g_steps_on_the_edge_shapes_match_the_restatement(name, d):
    user, samples, g_reg = G_EDGES[name]
    M, tables = _edge(d)
    eng = _engine(tables, M, lr=0.05, g_reg=g_reg, d_reg=0.0)
    r64, r32 = _pair(M, tables, g_reg, 0.0)
    for r in (r64, r32):
        r.g_step(user, samples)
    eng.g_step(user, samples)
    now = eng.tables()
    for k in ("g_P", "g_Q", "g_b"):
        _close(now[k], r64.T[k], np.abs(r32.T[k].astype(np.float64) - r64.T[k]).max(), "%s d=%d %s" % (name, d, k))
    others = np.arange(N_U) != user
    assert np.array_equal(now["g_P"][others], tables["g_P"][others])
    assert all(np.array_equal(now[k], tables[k]) for k in ("d_P", "d_Q", "d_b"))
    again = _engine(tables, M, lr=0.05, g_reg=g_reg, d_reg=0.0)
    again.g_step(user, samples)
    assert all(np.array_equal(v, now[k]) for k, v in again.tables().items())        # reruns are bit-identical


# ------------------------------------------------------------------ refusals, empty work, the drop-in run
def test_refusals_and_empty_work():
    import torch
    M, tables = _edge(20)
    eng = _engine(tables, M)
    before = eng.tables()
    eng.d_step([], [], [])
    eng.g_step(5)                                                   # a user without a train item
    eng.d_pass([], data=tuple(torch.zeros(0, dtype=dt, device=eng.dev) for dt in (torch.int32, torch.int32, torch.float32)))
    assert all(np.array_equal(v, before[k]) for k, v in eng.tables().items())
    empty = _engine(tables, sp.csr_matrix((N_U, N_I), dtype=np.float32))            # no train users
    assert len(empty.train_users) == 0 and empty.d_pass_size() == 0
    assert all(t.numel() == 0 for t in empty.d_data())
    empty.d_pass([])
    empty.g_pass()
    assert empty.g_passes == 1 and all(np.array_equal(v, before[k]) for k, v in empty.tables().items())
    with pytest.raises(ValueError, match=r"user ids must lie in \[0, 6\)"):
        eng.d_step([6], [0], [1.0])
    with pytest.raises(ValueError, match=r"item ids must lie in \[0, 1100\)"):
        eng.d_step([0], [1100], [1.0])
    with pytest.raises(ValueError, match="must have one length"):
        eng.d_step([0, 1], [1], [1.0])
    with pytest.raises(ValueError, match="a batch of 1025 pairs, the engine takes up to 1024"):
        eng.d_step([0] * 1025, [1] * 1025, [1.0] * 1025)
    with pytest.raises(ValueError, match="3 samples for user 1, 2 deg = 2 expected"):
        eng.g_step(1, [1, 2, 3])
    with pytest.raises(ValueError, match=r"item ids must lie in \[0, 1100\)"):
        eng.g_step(1, [1, 1100])
    with pytest.raises(ValueError, match="the order must index the pass's"):
        eng.d_pass([0, 1])
    with pytest.raises(ValueError, match="must hold a non-zero entry"):
        eng.draws(np.zeros(4, np.uint32), 0, [1], 0, 0)
    with pytest.raises(NotImplementedError, match=r"factors_num=129 is not supported \(1 to 128\)"):
        _engine(P.init_tables(N_U, N_I, 129, 1), M)
    with pytest.raises(NotImplementedError, match="batch_size=1025"):
        _engine(tables, M, batch=1025)
    with pytest.raises(ValueError, match=r"g_Q must be \[1100, 20\]"):
        _engine(dict(tables, g_Q=tables["g_Q"][:50]), M)
    assert torch.isfinite(eng.score([0, 5]).cpu()).all()


def test_irgan_config_drops_in(tmp_path):
    """NeuRec.properties + conf/IRGAN.properties on ml-100k through neurec_amd.main in a fresh child process, two
    epochs at the defaults but for a wider batch: no pretrain file, so the one log line saying so; one result line per G
    pass; the pass counters of the schedule; finite tables; predict() in both modes"""
    code = r"""
import json, os, re, sys
import numpy as np
sys.path.insert(0, %r)
from test_gru4rec_gpu import _run
tmp = %r
model = _run(tmp, ["--recommender=IRGAN", "--epochs=2", "--batch_size=512", "--lr=0.01"])
folder = os.path.join(tmp, "log", "ml-100k", "IRGAN")
files = os.listdir(folder)
text = open(os.path.join(folder, files[0])).read()
eng = model.engine
T = eng.tables()
cand = model.predict([0, 1], [[1, 2, 3], [4]])
full = model.predict([0, 1], None).cpu().numpy()
out = dict(files=len(files), absent=text.count("does not exist; the generator starts from uniform"),
           params="IRGAN's hyperparameters:" in text, passes=[eng.d_passes, eng.g_passes],
           finite=bool(all(np.isfinite(v).all() for v in T.values())), moved=bool(np.abs(T["g_b"]).max() > 0),
           scores=list(full.shape), users=int(len(eng.train_users)), items=eng.num_items,
           cand=[len(c) for c in cand], same=bool(np.allclose(cand[0], full[0, [1, 2, 3]], atol=1e-5)),
           results=len([ln for ln in text.splitlines() if re.search(r"\d\.\d{8}\s+\d\.\d{8}", ln)]))
print("RESULT " + json.dumps(out))
""" % (os.path.dirname(os.path.abspath(__file__)), str(tmp_path))
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    res = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["files"] == 1 and res["absent"] == 1 and res["params"], res
    assert res["passes"] == [2, 2] and res["finite"] and res["moved"], res
    assert res["scores"] == [2, res["items"]] and res["cand"] == [3, 1] and res["same"] and res["users"] > 900, res
    assert res["results"] == 2, res
