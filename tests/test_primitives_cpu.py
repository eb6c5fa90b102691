"""The restatement of the shared training primitives (tests/primitives_restatement.py) checked on the host: against
oracle.train.RowOptimizer bit for bit, the two RMSProp forms told apart, the constructed inputs of
test_primitives_gpu.py shown to hold what their names claim, and the float32-to-float64 distance of every case whose
GPU bound is a multiple of it shown to be non-zero."""
import numpy as np
import pytest

from oracle import train
import primitives_restatement as R


@pytest.mark.parametrize("kind", ["gd", "adagrad", "rmsprop", "momentum"])
def test_sparse_restatement_equals_the_oracle_row_optimizer(kind):
    """three steps on a 37 x 65 table with the slots carried: var, slot0 and slot1 bit-equal to oracle.train.RowOptimizer
    (TF's initial slots, rho 0.9, momentum 0 under rmsprop and 0.9 under momentum, epsilon 1e-10), rows outside the
    batch untouched"""
    rs = np.random.RandomState(3)
    shape, lr = (37, 65), 0.05
    var = rs.randn(*shape).astype(np.float32)
    opt = train.RowOptimizer(kind, lr, shape)
    want = var.copy()
    s0 = np.zeros(shape, np.float32) if opt.s0 is None else opt.s0.copy()
    s1 = np.zeros(shape, np.float32)
    h1, h2, eps = {"gd": (0, 0, 0), "adagrad": (0, 0, 0), "rmsprop": (0.9, 0.0, 1e-10), "momentum": (0.9, 0, 0)}[kind]
    for step in range(3):
        flag = R.flag_pattern("some", shape[0], rs)
        g = (0.1 * rs.randn(*shape)).astype(np.float32) * flag[:, None]
        rows = np.flatnonzero(flag)
        assert 0 < len(rows) < shape[0]
        before = var.copy()
        opt.apply(want, g, np.r_[rows, rows[:3]])                # repeats: the oracle takes the unique rows
        grad = g.copy()
        R.optimizer_rows(kind, var, s0, s1, grad, flag, lr, h1, h2, eps)
        assert np.array_equal(var, want), step
        if opt.s0 is not None:
            assert np.array_equal(s0, opt.s0), step
        if opt.s1 is not None:
            assert np.array_equal(s1, opt.s1), step
        still = np.setdiff1d(np.arange(shape[0]), rows)
        assert np.array_equal(var[still], before[still]) and not np.array_equal(var[rows], before[rows])
        assert not grad.any() and not flag.any()


def test_dense_and_sparse_rmsprop_are_two_forms():
    """the same table, slots and gradient, every row flagged: ApplyRMSProp (moving average as an increment, the step a
    division) and SparseApplyRMSProp (a blend, the step a reciprocal square root) give different float32 bits, with
    and without momentum, and agree in float64 to rounding — neither may stand in for the other"""
    shape = (37, 65)
    for h2 in (0.0, 0.5):
        var, s0, s1 = R.optimizer_inputs("rmsprop", shape, 5)
        g = (0.1 * np.random.RandomState(6).randn(*shape)).astype(np.float32)
        out = {}
        for dt in (np.float32, np.float64):
            a = [x.astype(dt) for x in (var, s0, s1, g)]
            b = [x.astype(dt) for x in (var, s0, s1, g)]
            R.optimizer_rows("rmsprop", *a, np.ones(shape[0], np.uint8), 0.05, 0.9, h2, 1e-10)
            R.optimizer_dense("rmsprop", *b, 0.05, 0.9, h2, 1e-10)
            out[dt] = (a, b)
        a, b = out[np.float32]
        for k, name in enumerate(("var", "ms", "mom")):
            assert not np.array_equal(a[k], b[k]), name
            assert np.abs(out[np.float64][0][k] - out[np.float64][1][k]).max() <= 1e-12, name
        assert not a[3].any() and np.array_equal(b[3], g)      # the sparse form clears its gradient rows


def test_dense_restatement_clears_only_on_request():
    var, s0, s1 = R.optimizer_inputs("momentum", (257,), 1)
    g = np.ones(257, np.float32)
    R.optimizer_dense("momentum", var, s0, s1, g, 0.1, 0.9, clear_grad=False)
    assert g.all()
    R.optimizer_dense("momentum", var, s0, s1, g, 0.1, 0.9, clear_grad=True)
    assert not g.any()


def _runs(users, items, third):
    return R.run_lengths(R.host_plan(users, items, third, R.MF_USERS))


def test_constructed_batches_hold_what_they_claim():
    """on the host-sorted plan: user 0's run is sorted positions 0 .. 15 (workgroup 0 exactly) and 0 .. 31 (two
    workgroups exactly); user 11's run is 40 long, starts inside workgroup 0 and ends inside workgroup 2, so workgroup 1
    is all of one row with the run going on at both edges; item 7's run is 42 long pairwise — 21 positive lookups (slot
    40 among them) before 21 negative lookups (slot 40 again) — and 21 pointwise"""
    W = R.OCC_PER_WORKGROUP
    for name, length in (("run16", 16), ("run32", 32)):
        users, items, negs = R.constructed_batch(name)
        assert len(users) == 64 and (users == 0).sum() == length and users.min() == 0
        for third in (negs, None):
            assert _runs(users, items, third)[0] == (0, 0, length)
            assert _runs(users, items, third)[1][1] == length and length % W == 0
    users, items, negs = R.constructed_batch("run40")
    for third in (negs, None):
        row, start, length = [r for r in _runs(users, items, third) if r[0] == R.RUN40_USER][0]
        assert length == 40 and start % W != 0 and start // W == 0 and (start + length - 1) // W == 2
        assert (start + length) % W != 0
    users, items, negs = R.constructed_batch("item_both")
    both = np.flatnonzero((items == R.BOTH_ITEM) & (negs == R.BOTH_ITEM))
    assert (items == R.BOTH_ITEM).sum() == 21 and (negs == R.BOTH_ITEM).sum() == 21 and len(both) == 1
    plan = R.host_plan(users, items, negs, R.MF_USERS)
    row, start, length = [r for r in R.run_lengths(plan) if r[0] == R.MF_USERS + R.BOTH_ITEM][0]
    assert length == 42
    p = plan[start:start + length] & 0xffffffff
    assert np.all(p[:21] // 64 == 1) and np.all(p[21:] // 64 == 2)          # the positives first, both in slot order
    assert np.all(np.diff(p) > 0) and both[0] in p[:21] % 64 and both[0] in p[21:] % 64
    assert start // W != (start + length - 1) // W
    assert [r for r in _runs(users, items, None) if r[0] == R.MF_USERS + R.BOTH_ITEM][0][2] == 21


def test_batch_sizes_sit_on_both_sides_of_a_workgroup():
    W = R.OCC_PER_WORKGROUP
    assert 3 * 5 < W < 3 * 6 and 2 * 6 < W and 2 * 33 > 4 * W and 1 in R.MF_BATCHES
    assert {d <= 64 for d in R.MF_DIMS} == {True, False} and {64, 65, 128, 129, 256} <= set(R.MF_DIMS)


def test_hinge_kink_is_exact():
    """triplet 0 sits exactly on the kink (y + 1 == 0 in float32 and in float64) and takes derivative 0; the float32
    restatement of the whole case equals the float64 one exactly, so the device can be held to its bits"""
    P, Q, users, pos, neg, reg = R.hinge_kink()
    for dt in (np.float32, np.float64):
        p, qi, qj = P.astype(dt)[users], Q.astype(dt)[pos], Q.astype(dt)[neg]
        y = np.sum(p * qi, axis=1, dtype=dt) - np.sum(p * qj, axis=1, dtype=dt)
        assert y.dtype == dt and y[0] + dt(1) == 0 and y[1] + dt(1) == 1.0625
        assert train.pairwise_terms("hinge", y)[1].tolist() == [0.0, 1.0]
    l32, r32, dP32, dQ32 = R.mf_gradients(P, Q, users, pos, neg, True, "hinge", np.float32, reg)
    l64, r64, dP64, dQ64 = R.mf_gradients(P, Q, users, pos, neg, True, "hinge", np.float64, reg)
    assert l32 == l64 == 1.0625 and r32 == r64
    assert np.array_equal(dP32.astype(np.float64), dP64) and np.array_equal(dQ32.astype(np.float64), dQ64)
    assert np.array_equal(dP64[1], reg * P[1].astype(np.float64))          # the kink slot: the regulariser alone
    assert not dP64[2].any() and not dQ64[1].any()


def test_float32_restatement_differs_from_float64_in_every_mf_case():
    """the GPU bound is 4 x (float32 restatement's distance to float64) + 1e-5 max|want| per case and array: the
    distance is non-zero for both gradient tables and the regulariser in every case, and for the data loss in every
    case but those where it is exactly 0 in both widths (a hinge batch with every slot cut: only B = 1 can be)"""
    n = 0
    for case in R.mf_cases():
        c = R.mf_case(*case)
        for k, name in enumerate(("loss", "reg", "dP", "dQ")):
            w32, w64 = np.asarray(c["f32"][k], np.float64), np.asarray(c["f64"][k])
            if name == "loss" and not w64.any():
                assert case[1] == "hinge" and case[3] == 1 and not w32.any(), case
                continue
            assert np.abs(w32 - w64).max() > 0, (case, name)
        n += 1
    assert n == len(R.MF_LOSSES) * (len(R.MF_DIMS) * len(R.MF_BATCHES) + len(R.MF_CONSTRUCTED_DIMS) * 4)


def test_float32_row_sums_differ_from_float64_wherever_something_is_added():
    """every case with a run of two or more has a non-zero float32-to-float64 distance; n = 1 is a copy, exact in both
    (the GPU test holds it to bit equality like the rest).  The runs are the ones the names claim."""
    for d in R.ROWSUM_DIMS:
        for n in R.ROWSUM_NS:
            c = R.rowsum_case(d, n)
            lengths = [r[2] for r in R.run_lengths(c["keys"])]
            assert sum(lengths) == n and np.all(np.diff(c["keys"]) > 0)
            assert sorted(c["index_of_pos"].tolist()) == list(range(n))
            if n == 300:
                assert 70 in lengths and 1 in lengths and len(c["rows"]) < R.ROWSUM_ROWS
            for s in ("a", "b"):
                w32, w64 = c["f32_" + s].astype(np.float64), c["f64_" + s]
                still = np.setdiff1d(np.arange(R.ROWSUM_ROWS), c["rows"])
                assert len(still) and np.all(w64[still] == R.ROWSUM_CANARY)
                assert (np.abs(w32 - w64).max() > 0) == (max(lengths) > 1), (d, n, s)


def test_sort_inputs_hold_duplicates_and_the_largest_key():
    for n in R.SORT_NS:
        keys = R.sort_keys_input(n)
        assert len(keys) == n and (n == 0 or (keys.max() == 0x7fffffffffffffff and keys.min() >= 0))
        if n >= 63:
            assert len(np.unique(keys >> 32)) <= 8 and len(np.unique(keys)) < n
