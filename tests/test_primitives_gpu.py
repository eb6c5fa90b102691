"""The shared training primitives called directly (csrc/adam.hip, csrc/bpr.hip and the small reductions of
csrc/vae.hip through the neurec_amd.engine wrappers) against tests/primitives_restatement.py: bit equality with the
float32 restatement wherever the arithmetic order is documented, the float64 restatement within
4 x (float32 restatement's own distance) + 1e-5 max|want| for the MF gradients and the ordered row sums, canaries
around every strided view and in every row or element a call must leave alone."""
import ctypes as C
import math

import numpy as np
import pytest

import primitives_restatement as R

pytestmark = pytest.mark.gpu

CANARY = 7.0
WORST = {}              # section -> largest device err / reference f32 err seen


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                # a copy: the shared cases are read-only


def _np(t):
    return t.cpu().numpy()


def _bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), \
        (what, int((got != want).sum()), float(np.abs(got.astype(np.float64) - want).max()) if got.size else 0.0)


def _within(section, what, got, w32, w64):
    """device err <= 4 x reference f32 err + 1e-5 max|want|, printed as test_hrm_gpu.py prints it"""
    got, w32, w64 = (np.asarray(x, np.float64) for x in (got, w32, w64))
    err, bar = np.abs(got - w64).max(), np.abs(w32 - w64).max()
    if bar > 0:
        WORST[section] = max(WORST.get(section, 0.0), err / bar)
    print("%s: device err %.3g, reference f32 err %.3g (largest ratio of %s so far %.3g)"
          % (what, err, bar, section, WORST.get(section, 0.0)))
    assert err <= 4 * bar + 1e-5 * np.abs(w64).max(), (what, err, bar)


# ================================================================== 1. the MF gradient kernels
def _mf_call(E, c, pairwise, kind, plan, reg=R.MF_REG, fill=CANARY):
    import torch
    P, Q, users, items, third = (_dev(c[k]) for k in ("P", "Q", "users", "items", "third"))
    B = len(c["users"])
    GP, GQ = torch.full_like(P, fill), torch.full_like(Q, fill)
    terms, loss2 = torch.empty(8 * B, device="cuda"), torch.full((2,), fill, device="cuda")
    fn = E.pairwise_mf_grad if pairwise else E.pointwise_mf_grad
    fn(P, Q, users, items, third, reg, kind, GP, GQ, terms, loss2, plan=plan)
    return _np(loss2), _np(GP), _np(GQ)


def _mf_check(pairwise, kind, d, batch):
    from neurec_amd import engine as E
    c = R.mf_case(pairwise, kind, d, batch)
    users, items, third = (_dev(c[k]) for k in ("users", "items", "third"))
    plan = E.bpr_plan(users, items, third if pairwise else None, len(c["users"]), R.MF_USERS)
    _bits(_np(plan), c["plan"], "plan")
    runs = [_mf_call(E, c, pairwise, kind, p) for p in (None, plan, None)]
    for other in runs[1:]:                                    # own plan, given plan, and again: the same bits
        for a, b in zip(runs[0], other):
            _bits(a, b, "repeat")
    loss2, GP, GQ = runs[0]
    l32, r32, dP32, dQ32 = c["f32"]
    l64, r64, dP64, dQ64 = c["f64"]
    tag = "%s %s d=%d B=%s" % ("pairwise" if pairwise else "pointwise", kind, d, batch)
    _within("mf", tag + " loss", loss2[0], l32, l64)
    _within("mf", tag + " reg", loss2[1], r32, r64)
    for name, G, rows, w32, w64 in (("GP", GP, c["rows_P"], dP32, dP64), ("GQ", GQ, c["rows_Q"], dQ32, dQ64)):
        still = np.setdiff1d(np.arange(len(G)), rows)
        _bits(G[still], np.full((len(still), d), CANARY, np.float32), tag + " untouched " + name)
        # stored, not added: the 7.0 a touched row held is gone
        _within("mf", tag + " " + name, G[rows], w32[rows], w64[rows])


@pytest.mark.parametrize("d", R.MF_DIMS)
@pytest.mark.parametrize("pairwise,kind", R.MF_LOSSES)
def test_mf_gradients_against_float64(pairwise, kind, d):
    """U = 23, I = 31, B = 1, 5, 6, 33, 71 random slots, gradient only: loss2[0], loss2[1] and the touched rows of GP
    and GQ against the float64 restatement; GP and GQ start at 7.0 everywhere — touched rows hold the gradient (a
    store), every other row is still 7.0 bit for bit; the device's own plan equals the host-sorted one; plan=None,
    plan=bpr_plan(...) and a second call give identical bits"""
    for B in R.MF_BATCHES:
        _mf_check(pairwise, kind, d, B)


@pytest.mark.parametrize("d", R.MF_CONSTRUCTED_DIMS)
@pytest.mark.parametrize("pairwise,kind", R.MF_LOSSES)
def test_mf_gradients_on_constructed_runs(pairwise, kind, d):
    """B = 64 with one row's run filling workgroup 0 exactly, two workgroups exactly, 40 occurrences with a whole
    workgroup in the middle, and one item 21 times positive and 21 times negative (test_primitives_cpu.py holds the
    batches to these claims): the same checks"""
    for name in R.MF_CONSTRUCTED:
        _mf_check(pairwise, kind, d, name)


def test_hinge_kink_bit_exact():
    """the dyadic two-triplet case with y + 1 == 0 exactly: derivative 0 there, loss and gradients bit-equal to the
    restatement (float32 and float64 agree exactly: test_primitives_cpu.py)"""
    from neurec_amd import engine as E
    P, Q, users, pos, neg, reg = R.hinge_kink()
    c = {"P": P, "Q": Q, "users": users, "items": pos, "third": neg}
    loss2, GP, GQ = _mf_call(E, c, True, "hinge", None, reg=reg)
    l, r, dP, dQ = R.mf_gradients(P, Q, users, pos, neg, True, "hinge", np.float32, reg)
    assert loss2.tolist() == [float(l), float(r)] and float(l) == 1.0625
    _bits(GP[:2], dP[:2], "GP")
    _bits(GQ[[0, 2, 3]], dQ[[0, 2, 3]], "GQ")
    _bits(GP[1], np.float32(reg) * P[1], "the kink slot: the regulariser alone")
    assert np.all(GP[2] == CANARY) and np.all(GQ[1] == CANARY)


@pytest.mark.parametrize("pairwise,kind", [(True, "bpr"), (False, "square")])
def test_mf_gradients_of_an_empty_batch(pairwise, kind):
    """batch == 0 (an empty slice of a stream; an empty tensor has no storage, its data_ptr() is NULL): loss2 is zeroed,
    GP, GQ and the work buffer are not touched"""
    import torch
    from neurec_amd import engine as E
    P, Q = (_dev(x) for x in R.mf_tables(20))
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    third = ids if pairwise else torch.zeros(4, device="cuda")
    GP, GQ = torch.full_like(P, CANARY), torch.full_like(Q, CANARY)
    terms, loss2 = torch.full((8,), CANARY, device="cuda"), torch.full((2,), CANARY, device="cuda")
    fn = E.pairwise_mf_grad if pairwise else E.pointwise_mf_grad
    fn(P, Q, ids[:0], ids[:0], third[:0], 0.01, kind, GP, GQ, terms, loss2)
    assert _np(loss2).tolist() == [0.0, 0.0]
    assert bool((GP == CANARY).all()) and bool((GQ == CANARY).all()) and bool((terms == CANARY).all())


# ================================================================== 2. optimizer_rows
def _rows_case(kind, h1, h2, eps, n_rows, d, pattern, last_rows_flagged=0):
    from neurec_amd import engine as E
    lr = 0.05
    rs = np.random.RandomState(n_rows + 1000 * d + len(pattern))
    var, s0, s1 = R.optimizer_inputs(kind, (n_rows, d), d + n_rows)
    dvar, ds0, ds1 = _dev(var), _dev(s0), _dev(s1)
    for step in range(3):
        flag = R.flag_pattern(pattern, n_rows, rs)
        if last_rows_flagged:
            flag[-last_rows_flagged:] = 1
        g = (0.1 * rs.randn(n_rows, d)).astype(np.float32)          # non-zero in unflagged rows too: they must keep it
        dg, dflag = _dev(g), _dev(flag)
        before = [x.copy() for x in (var, s0, s1, g)]
        still = np.flatnonzero(flag == 0)
        flagged = np.flatnonzero(flag)
        E.optimizer_rows(kind, dvar, ds0, ds1, dg, dflag, lr, h1, h2, eps)
        R.optimizer_rows(kind, var, s0, s1, g, flag, lr, h1, h2, eps)
        what = (kind, h2, n_rows, d, pattern, step)
        for name, dev, want, was in (("var", dvar, var, before[0]), ("slot0", ds0, s0, before[1]),
                                     ("slot1", ds1, s1, before[2]), ("grad", dg, g, before[3])):
            got = _np(dev)
            _bits(got, want, what + (name,))
            _bits(got[still], was[still], what + (name, "unflagged rows"))
        assert not _np(dg)[flagged].any() and not _np(dflag).any(), what
        if len(flagged):
            assert not np.array_equal(var[flagged], before[0][flagged]), what


@pytest.mark.parametrize("kind,h1,h2,eps", R.OPTIMIZERS)
def test_optimizer_rows_bit_exact(kind, h1, h2, eps):
    """d = 1, 63, 64, 65, 130 x 1, 5, 37 rows x no / every / about 40 % of the rows flagged, three steps with the slots
    carried (RMSProp also with momentum 0.5): var, slot0 and slot1 bit-equal to the float32 restatement, unflagged rows
    of all four buffers bit-untouched, flagged gradient rows and every flag zero afterwards"""
    for d in (1, 63, 64, 65, 130):
        for n_rows in (1, 5, 37):
            for pattern in ("none", "all", "some"):
                _rows_case(kind, h1, h2, eps, n_rows, d, pattern)


@pytest.mark.parametrize("kind,h1,h2,eps", R.OPTIMIZERS)
def test_optimizer_rows_second_grid_stride_pass(kind, h1, h2, eps):
    """4 * 8192 + 3 rows at d = 1: the grid is capped at 8,192 workgroups of four rows, the last three rows (flagged)
    are reached only by a second iteration of the grid-stride loop"""
    _rows_case(kind, h1, h2, eps, 4 * 8192 + 3, 1, "some", last_rows_flagged=3)


# ================================================================== 3. DenseLearner / nrhip_optimizer_dense_tf
def _dense_apply(E, kind, lr, h1, h2, eps, var, s0, s1, grad, clear):
    if kind != "rmsprop" or h2 == 0.0:                        # what DenseLearner passes: (0.9, 0, 1e-10) under rmsprop
        E.DenseLearner(kind, lr, momentum=h1 if kind == "momentum" else 0.9).apply([(var, s0, s1, grad, clear)])
    else:
        E.call("nrhip_optimizer_dense_tf", E.ROW_OPTIMIZERS[kind], E._ptr(var), E._ptr(s0), E._ptr(s1), E._ptr(grad),
               var.numel(), lr, h1, h2, eps, clear, E._stream())


@pytest.mark.parametrize("kind,h1,h2,eps", R.OPTIMIZERS)
def test_dense_optimizer_bit_exact(kind, h1, h2, eps):
    """n = 1, 255, 256, 257 and 256 * 8192 + 5 (the grid is capped at 8,192 workgroups: a second grid-stride pass), with
    and without the gradient clear, three steps: var and both slots bit-equal to the float32 restatement of TF's dense
    Apply* kernels; the gradient is zero (clear) or untouched"""
    from neurec_amd import engine as E
    lr = 0.05
    for n in (1, 255, 256, 257, 256 * 8192 + 5):
        for clear in (0, 1):
            rs = np.random.RandomState(n % 1000 + clear)
            var, s0, s1 = R.optimizer_inputs(kind, (n,), n % 977)
            dvar, ds0, ds1 = _dev(var), _dev(s0), _dev(s1)
            for step in range(3):
                g = (0.1 * rs.randn(n)).astype(np.float32)
                dg = _dev(g)
                _dense_apply(E, kind, lr, h1, h2, eps, dvar, ds0, ds1, dg, clear)
                g_after = g.copy()
                R.optimizer_dense(kind, var, s0, s1, g_after, lr, h1, h2, eps, clear_grad=bool(clear))
                what = (kind, h2, n, clear, step)
                for name, dev, want in (("var", dvar, var), ("slot0", ds0, s0), ("slot1", ds1, s1), ("grad", dg, g_after)):
                    _bits(_np(dev), want, what + (name,))
                assert g_after.any() != bool(clear)


def test_dense_learner_initial_slots():
    """init_slots: what TF creates the slots with — adagrad's accumulator 1e-8 (learner.py:5-6), rmsprop's `rms` ones
    and `momentum` zeros, momentum's accumulator zeros"""
    import torch
    from neurec_amd import engine as E
    for kind, v0 in (("gd", 0.0), ("adagrad", 1e-8), ("rmsprop", 1.0), ("momentum", 0.0)):
        a = [torch.full((n,), CANARY, device="cuda") for n in (5, 257)]
        b = [torch.full((n,), CANARY, device="cuda") for n in (5, 257)]
        E.DenseLearner(kind, 0.1).init_slots(a, b)
        for t in a:
            _bits(_np(t), np.full(t.numel(), v0, np.float32), kind)
        for t in b:
            assert not _np(t).any()
    with pytest.raises(ValueError, match="suitable optimizer"):
        E.DenseLearner("adam", 0.1)


# ================================================================== 4. adam_dense_multi
MULTI_SIZES = [0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 4099, 6, 7, 8, 9, 12, 13, 31, 33, 63, 64, 65, 100, 255, 256, 257,
               1000, 2047, 2048, 2049, 4096, 4097, 5000]


def _adam_inputs(n, rs):
    f = lambda a: np.asarray(a, np.float32)
    return [f(rs.randn(n)), f(1e-2 * rs.randn(n)), f(1e-3 * rs.rand(n)), f(0.1 * rs.randn(n))]


def test_adam_dense_multi_equals_single_launches_and_the_oracle():
    """32 tensors of 0 .. 5,000 elements (every length mod 4, both sides of 1,024 float4s) with mixed clear flags in one
    launch: every tensor bit-equal to adam_dense on a copy and to oracle.train.Adam.dense, gradients zero where
    asked and untouched elsewhere"""
    from neurec_amd import engine as E
    from oracle import train
    assert len(MULTI_SIZES) == 32 and {n % 4 for n in MULTI_SIZES} == {0, 1, 2, 3}
    rs = np.random.RandomState(4)
    st, ad = E.AdamState(0.001), train.Adam(0.001)
    for _ in range(4):
        st.advance(); ad.advance()
    host = [_adam_inputs(n, rs) for n in MULTI_SIZES]
    clear = [k % 3 != 1 for k in range(32)]
    multi = [[_dev(x) for x in t] for t in host]
    single = [[_dev(x) for x in t] for t in host]
    E.adam_dense_multi([tuple(t) + (c,) for t, c in zip(multi, clear)], st)
    for k, (n, c) in enumerate(zip(MULTI_SIZES, clear)):
        E.adam_dense(*single[k], st, clear_grad=c)
        var, m, v, g = (x.copy() for x in host[k])
        ad.dense(var, m, v, g)
        want = [var, m, v, np.zeros_like(g) if c else g]
        for name, a, b, w in zip(("var", "m", "v", "grad"), multi[k], single[k], want):
            _bits(_np(a), w, (k, n, name, "multi vs oracle"))
            _bits(_np(b), w, (k, n, name, "single vs oracle"))


def test_adam_dense_multi_refusals():
    """33 tensors in one call to the C entry point are refused (the wrapper cuts its list into launches of 32), and a
    view that starts 4 bytes into an allocation is refused with the alignment message"""
    import torch
    from neurec_amd import engine as E
    st = E.AdamState(0.001)
    n = 33
    bufs = [[torch.zeros(8, device="cuda") for _ in range(4)] for _ in range(n)]
    arr = lambda i: (C.c_void_p * n)(*[t[i].data_ptr() for t in bufs])
    sizes, clear = (C.c_int64 * n)(*([8] * n)), (C.c_int32 * n)(*([0] * n))
    with pytest.raises(ValueError, match=r"0\.\.32 tensors"):
        E.call("nrhip_adam_dense_tf_multi", n, arr(0), arr(1), arr(2), arr(3), sizes, clear, st.alpha(), st.beta1,
               st.beta2, st.eps, E._stream())
    E.adam_dense_multi([tuple(t) for t in bufs], st)                          # 32 + 1 through the wrapper
    big = [torch.zeros(16, device="cuda") for _ in range(4)]
    for k in range(4):
        t = [x[1:] if j == k else x[:15] for j, x in enumerate(big)]
        with pytest.raises(ValueError, match="16-byte aligned"):
            E.adam_dense_multi([tuple(t)], st)
    assert not any(x.any().item() for x in big)


# ================================================================== 5. the row movers
N_TABLE = 50
LISTED = (0, 1, 4, 5, 133)          # 133 > 50 rows: repeats; 4 / 5: one workgroup of four waves and one wave more
ROW_DIMS = (1, 64, 65, 200)


def _wide(rows, d, pad, rs=None, fill=CANARY):
    """a [rows][d + pad] buffer of canaries and its column block [:, 2 : 2 + d] (row stride d + pad, 8 bytes into the
    row), filled with random values when rs is given"""
    import torch
    wide = torch.full((rows, d + pad), fill, device="cuda")
    view = wide[:, 2:2 + d]
    if rs is not None:
        view.copy_(_dev(rs.randn(rows, d).astype(np.float32)))
    return wide, view


def _padding_intact(wide, d):
    w = _np(wide)
    return bool(np.all(w[:, :2] == CANARY) and np.all(w[:, 2 + d:] == CANARY))


def _listed(rs, n):
    rows = rs.randint(0, N_TABLE, n).astype(np.int32)
    if n > N_TABLE:
        assert len(np.unique(rows)) < n
    return rows


@pytest.mark.parametrize("d", ROW_DIMS)
def test_rows_gather_between_column_blocks(d):
    """rows_gather and rows_gather2 with 0, 1, 4, 5 and 133 listed rows (repeats), every source and destination a
    column block of a wider buffer (row strides d + 3 and, for the second pair, d + 5): the listed rows arrive, the
    padding of the destinations keeps its canary, the sources are unchanged"""
    from neurec_amd import engine as E
    rs = np.random.RandomState(d)
    for n in LISTED:
        rows = _listed(rs, n)
        src_w, src = _wide(N_TABLE, d, 3, rs)
        srcb_w, srcb = _wide(N_TABLE, d, 5, rs)
        keep = _np(src_w).copy(), _np(srcb_w).copy()
        dst_w, dst = _wide(n, d, 3)
        E.rows_gather(_dev(rows), src, dst)
        _bits(_np(dst), _np(src)[rows], ("gather", d, n))
        assert _padding_intact(dst_w, d)
        da_w, da = _wide(n, d, 3)
        db_w, db = _wide(n, d, 5)
        E.rows_gather2(_dev(rows), src, srcb, da, db)
        _bits(_np(da), _np(src)[rows], ("gather2 a", d, n))
        _bits(_np(db), _np(srcb)[rows], ("gather2 b", d, n))
        assert _padding_intact(da_w, d) and _padding_intact(db_w, d)
        _bits(_np(src_w), keep[0], "source a")
        _bits(_np(srcb_w), keep[1], "source b")


@pytest.mark.parametrize("d", ROW_DIMS)
def test_rows_scatter_add_is_exact_on_dyadic_values(d):
    """multiples of 1/4 below 8 in magnitude: every partial sum of up to 134 of them is exact in float32, so the result
    is the same whatever order the atomics take and must be bit-equal to np.add.at; unlisted rows are untouched; the
    source is a column block of a wider buffer"""
    from neurec_amd import engine as E
    rs = np.random.RandomState(d + 1)
    for n in LISTED:
        rows = _listed(rs, n)
        vals = (rs.randint(-31, 32, (n, d)) / 4.0).astype(np.float32)
        src_w, src = _wide(n, d, 3)
        src.copy_(_dev(vals))
        want = (rs.randint(-31, 32, (N_TABLE, d)) / 4.0).astype(np.float32)
        dst = _dev(want)
        E.rows_scatter_add(_dev(rows), src, dst)
        before = want.copy()
        np.add.at(want, rows, vals)
        _bits(_np(dst), want, ("scatter_add", d, n))
        still = np.setdiff1d(np.arange(N_TABLE), rows)
        _bits(_np(dst)[still], before[still], ("scatter_add unlisted", d, n))
        assert _padding_intact(src_w, d)


@pytest.mark.parametrize("d", ROW_DIMS)
def test_rows_div_and_rows_clear(d):
    """rows_div: dst[r] = src[r] / 3 on the listed rows (a correctly rounded division, as numpy's), the others keep
    their canary.  rows_clear with 1, 2, 3 and 4 buffers, with and without a flag array: the listed rows and their
    flags are zero, every other row and flag is untouched"""
    import torch
    from neurec_amd import engine as E
    rs = np.random.RandomState(d + 2)
    for n in LISTED:
        rows = _listed(rs, n)
        drows = _dev(rows)
        still = np.setdiff1d(np.arange(N_TABLE), rows)
        src = rs.randn(N_TABLE, d).astype(np.float32)
        dsrc, dst = _dev(src), torch.full((N_TABLE, d), CANARY, device="cuda")
        E.rows_div(drows, dsrc, 3.0, dst)
        want = np.full((N_TABLE, d), CANARY, np.float32)
        want[rows] = src[rows] / np.float32(3.0)
        _bits(_np(dst), want, ("rows_div", d, n))
        _bits(_np(dsrc), src, "rows_div source")
        for n_bufs in (1, 2, 3, 4):
            for with_flag in (False, True):
                host = [rs.randn(N_TABLE, d).astype(np.float32) + 3.0 for _ in range(n_bufs)]
                bufs = [_dev(h) for h in host]
                flag = torch.ones(N_TABLE, dtype=torch.uint8, device="cuda") if with_flag else None
                E.rows_clear(drows, d, bufs, flag)
                for h, b in zip(host, bufs):
                    got = _np(b)
                    assert not got[rows].any(), ("rows_clear", d, n, n_bufs)
                    _bits(got[still], h[still], ("rows_clear unlisted", d, n, n_bufs))
                if with_flag:
                    f = _np(flag)
                    assert not f[rows].any() and np.all(f[still] == 1)


def test_mark_rows_and_gather_u8():
    """mark_rows with offset 0 and 9: flag[id + offset] = 1 and nothing else; gather_u8: dst[i] = src[index[i]]; both
    with 0, 1, 4, 5, 133 and 257 ids"""
    import torch
    from neurec_amd import engine as E
    rs = np.random.RandomState(9)
    for n in LISTED + (257,):
        ids = _listed(rs, n)
        for offset in (0, 9):
            flag = torch.zeros(N_TABLE + 9, dtype=torch.uint8, device="cuda")
            E.mark_rows(_dev(ids), flag, offset)
            want = np.zeros(N_TABLE + 9, np.uint8)
            want[ids.astype(np.int64) + offset] = 1
            _bits(_np(flag), want, ("mark_rows", n, offset))
        src = rs.randint(0, 256, N_TABLE).astype(np.uint8)
        dst = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
        E.gather_u8(_dev(src), _dev(ids), dst)
        _bits(_np(dst), src[ids], ("gather_u8", n))


# ================================================================== 6. sort_keys and the ordered row sums
@pytest.mark.parametrize("n", R.SORT_NS)
def test_sort_keys_in_one_workgroup(n):
    """the single-workgroup network of nrhip_sort_u64 (up to 16,384 keys) at every padded size's edge: keys with seven
    values in the high word, repeated whole keys and 0x7fffffffffffffff, against np.sort"""
    from neurec_amd import engine as E
    keys = R.sort_keys_input(n)
    got = E.sort_keys(_dev(keys.copy()))
    _bits(_np(got), np.sort(keys), n)


@pytest.mark.parametrize("d", R.ROWSUM_DIMS)
def test_rows_sum_sorted_in_key_order(d):
    """n = 1, 4, 5 and 300 keys (runs of 1 and 70 among them) over 40 destination rows, index_of_pos a random
    permutation, the sources column blocks of [n][d + 3] buffers: bit-equal to the float32 sum taken one row at a time
    in key order, within the bound of the float64 one; rows with keys are overwritten (the canary is gone), the others
    keep it; rows_sum_sorted2 equals two rows_sum_sorted calls bit for bit"""
    import torch
    from neurec_amd import engine as E
    for n in R.ROWSUM_NS:
        c = R.rowsum_case(d, n)
        keys, iop = _dev(c["keys"]), _dev(c["index_of_pos"])
        src_a, src_b = _dev(c["src_a"])[:, :d], _dev(c["src_b"])[:, :d]
        assert src_a.stride(0) == d + 3
        fresh = lambda: torch.full((R.ROWSUM_ROWS, d), R.ROWSUM_CANARY, device="cuda")
        one_a, one_b, two_a, two_b = fresh(), fresh(), fresh(), fresh()
        E.rows_sum_sorted(keys, iop, src_a, one_a)
        E.rows_sum_sorted(keys, iop, src_b, one_b)
        E.rows_sum_sorted2(keys, iop, src_a, two_a, src_b, two_b)
        for s, one, two in (("a", one_a, two_a), ("b", one_b, two_b)):
            got = _np(one)
            _bits(got, c["f32_" + s], ("rows_sum_sorted", d, n, s))
            _bits(_np(two), got, ("rows_sum_sorted2", d, n, s))
            _within("row sums", "rows_sum_sorted d=%d n=%d %s" % (d, n, s), got, c["f32_" + s], c["f64_" + s])
            still = np.setdiff1d(np.arange(R.ROWSUM_ROWS), c["rows"])
            assert np.all(got[still] == R.ROWSUM_CANARY) and not np.any(got[c["rows"]] == R.ROWSUM_CANARY)


# ================================================================== 7. element-wise helpers and reductions
EW_NS = (1, 255, 257, 4096 * 256 + 5)          # the last: beyond the 4,096-workgroup cap of the sweeps


@pytest.mark.parametrize("n", EW_NS)
def test_scale_add_div_scalar_equal_numpy(n):
    """scale, add and div_scalar against numpy float32 exactly, the inputs unchanged; scale also in place
    (out is x), as neurec_amd/replicas.py calls it — the one caller in the package that passes a tensor twice"""
    import torch
    from neurec_amd import engine as E
    rs = np.random.RandomState(n % 1000)
    x, y = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    dx, dy = _dev(x), _dev(y)
    fresh = lambda: torch.full((n,), CANARY, device="cuda")
    a = np.float32(0.37)
    out = fresh()
    E.scale(dx, 0.37, out)
    _bits(_np(out), a * x, "scale")
    out = fresh()
    E.add(dx, dy, out)
    _bits(_np(out), x + y, "add")
    out = fresh()
    E.div_scalar(dx, 3.0, out)
    _bits(_np(out), x / np.float32(3.0), "div_scalar")
    _bits(_np(dx), x, "x")
    _bits(_np(dy), y, "y")
    E.scale(dx, 0.37, dx)
    _bits(_np(dx), a * x, "scale in place")


@pytest.mark.parametrize("rows", [1, 5, 1000])
def test_add2d_and_copy2d_on_column_blocks(rows):
    """cols = 1, 7, 64 with row stride cols + 3 on every operand: the block holds x + y (numpy float32 exactly) or x,
    the padding keeps its canary, the inputs are unchanged"""
    from neurec_amd import engine as E
    rs = np.random.RandomState(rows)
    for cols in (1, 7, 64):
        x_w, x = _wide(rows, cols, 3, rs)
        y_w, y = _wide(rows, cols, 3, rs)
        hx, hy = _np(x), _np(y)
        out_w, out = _wide(rows, cols, 3)
        E.add2d(x, y, out)
        _bits(_np(out), hx + hy, ("add2d", rows, cols))
        assert _padding_intact(out_w, cols)
        out_w, out = _wide(rows, cols, 3)
        E.copy2d(x, out)
        _bits(_np(out), hx, ("copy2d", rows, cols))
        assert _padding_intact(out_w, cols) and _padding_intact(x_w, cols) and _padding_intact(y_w, cols)
        _bits(_np(x), hx, "x")
        _bits(_np(y), hy, "y")


@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_axpy_and_the_reductions_against_float64(n):
    """csrc/vae.hip.  axpy is one fused multiply-add per element: a single rounding of the exact a x + y, error
    <= 2^-24 |a x + y| (plus the float64 reference's own rounding, 2^-52 (|a x| + |y|)).  sumsq_accumulate, mean_f32
    and mean2_f32 accumulate in float64, so instead of the float32 summation bound (n - 1) 2^-24 sum|x_i| they are held
    to 2^-24 |result| (the one rounding to float32, or less: the sum of squares stays float64), plus the float64
    accumulation's own n 2^-53 sum|terms|, which matters only where a mean cancels"""
    import torch
    from neurec_amd import engine as E
    rs = np.random.RandomState(n % 1000)
    x, y = (0.3 + rs.randn(n)).astype(np.float32), rs.randn(n).astype(np.float32)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    u, u53 = 2.0 ** -24, 2.0 ** -53
    dx, dy = _dev(x), _dev(y)
    E.axpy(0.37, dx, dy)
    a64 = float(np.float32(0.37))
    want = a64 * x64 + y64
    err = np.abs(_np(dy).astype(np.float64) - want)
    print("axpy n=%d: largest err / (2^-24 |want|) %.3g" % (n, (err / (u * np.abs(want) + 1e-300)).max()))
    assert np.all(err <= u * np.abs(want) + 2 * u53 * (np.abs(a64 * x64) + np.abs(y64)))
    _bits(_np(dx), x, "axpy x")

    acc = torch.full((1,), 1.5, dtype=torch.float64, device="cuda")
    E.sumsq_accumulate(dx, acc)
    want = math.fsum(x64 * x64)
    got = float(_np(acc)[0]) - 1.5
    print("sumsq n=%d: err %.3g, bound %.3g" % (n, abs(got - want), u * want))
    assert abs(got - want) <= u * want
    E.sumsq_accumulate(dx, acc)                                   # accumulates: twice the sum on top of 1.5
    assert abs(float(_np(acc)[0]) - 1.5 - 2 * want) <= 2 * u * want

    out1, out2 = torch.full((1,), CANARY, device="cuda"), torch.full((2,), CANARY, device="cuda")
    E.mean_f32(dx, out1)
    E.mean2_f32(dx, _dev(y), out2)
    for name, got, v in (("mean_f32", _np(out1)[0], x64), ("mean2_f32[0]", _np(out2)[0], x64),
                         ("mean2_f32[1]", _np(out2)[1], y64)):
        want = math.fsum(v) / n
        bound = u * abs(want) + n * u53 * np.abs(v).sum() / n
        print("%s n=%d: err %.3g, bound %.3g" % (name, n, abs(float(got) - want), bound))
        assert abs(float(got) - want) <= bound, name
    assert _np(out1)[0] == _np(out2)[0]                          # "same arithmetic as mean_kernel"
