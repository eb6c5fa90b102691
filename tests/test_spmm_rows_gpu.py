"""Every row of the sparse product, hub rows included, in bits against the order of additions the plan dictates.

For every (graph case, width, planner options) combination of tests/spmm_restatement.py::COMBOS the host planner
(tests/spmm_plan_host.py) builds the schedule, nrhip_spmm_blocked_plan_create builds it on the device with the same
explicit options, the two are shown byte-equal (same_plan), and every kernel form that runs the plan is compared with
the numpy walk of that very plan (spmm_restatement.lane_group / wanted_rows / wanted_wave): uint8 views, all rows.  Where
the planner refuses a combination the device entry must refuse it with the same message.  The work-item kernels of
spmm.hip are compared with spmm_restatement.work_item the same way.

Every form runs twice into fresh buffers and gives the same bits twice; every output buffer is pre-filled with a
canary and carries two canary rows beyond n_rows; rows a call must leave alone keep the canary.  All comparisons are
exact: there is no tolerance in this file."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import spmm_restatement as R
from spmm_plan_host import Refused, build, load_plancheck, same_plan

pytestmark = pytest.mark.gpu

CANARY = R.CANARY
BYTE_CANARY = 0xAA
_LIVE = []              # device tensors whose raw address went into a call, held until the test ends

ACCEPTED_64 = [c for c in R.COMBOS if c[1] == 64 and "refuse" not in c[3]]


@pytest.fixture(autouse=True)
def _hold_device_tensors_and_restore_the_knobs():
    """a call takes raw addresses, so nothing it was handed may be freed before it has run; the process-wide
    nrhip_spmm_blocked_tune* settings are back at their defaults for the next test whatever happened"""
    from neurec_amd import engine as E
    try:
        yield
    finally:
        import torch
        torch.cuda.synchronize()
        E.call("nrhip_spmm_blocked_tune", 8)
        E.call("nrhip_spmm_blocked_tune_packed", 1)
        E.call("nrhip_spmm_blocked_tune_addend_flag", 1)
        del _LIVE[:]


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()                   # a copy: the shared cases are read-only
    _LIVE.append(t)
    return t


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _np(t):
    return t.cpu().numpy()


def _bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got.view(np.uint8), want.view(np.uint8)):
        differ = got.view(np.uint8).reshape(got.shape[0], -1) != want.view(np.uint8).reshape(want.shape[0], -1)
        rows = np.flatnonzero(differ.any(1))
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64))))
        raise AssertionError((what, "%d elements in %d rows differ" % (int((got != want).sum()), len(rows)),
                              "rows", rows[:12].tolist(), "largest difference", worst))


def _rng(combo, salt):
    return np.random.RandomState(sum(map(ord, R.combo_id(combo))) * 31 + salt)


class _Ctx:
    """a combination on the device: the matrix, the host plan, the device plan shown equal to it, the packed pairs"""

    def __init__(self, combo, P, plan, buf):
        self.combo, self.P, self.plan, self.buf = combo, P, plan, buf
        self.name, self.d, self.n_wg, self.kw = combo
        self.case = R.case(self.name)
        self.A = self.case["A"]
        self.n, self.n_cols = self.A.shape
        self.idx, self.val = _dev(self.A.indices.astype(np.int32)), _dev(self.A.data.astype(np.float32))
        self.Xh = R.operand(self.case, self.d)
        rng = _rng(combo, 1)
        self.Hh, self.Sh, self.Lah, self.Lbh = (rng.randn(self.n, self.d).astype(np.float32) for _ in range(4))
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def main(self, keep=None):
        """the main schedule's rows (x_row_nonzero = keep: the operand zeroed where keep == 0, those terms skipped)"""
        if keep is None:
            return self.memo("main", lambda: R.lane_group(self.P, self.A, self.Xh))
        return self.memo(("main", keep.tobytes()),
                         lambda: R.lane_group(self.P, self.A, R.zero_rows(self.Xh, keep), x_row_nonzero=keep))

    def row_masked(self):
        """the rows as the kernel the row-masked hop reaches computes them"""
        k = R.dispatch(self.P, "rows")
        if k == "spmm_wanted_wave_kernel":
            return self.memo("ww", lambda: R.wanted_wave(self.P, self.A, self.Xh))
        if k == "spmm_wanted_rows_kernel":
            return self.memo("w", lambda: R.wanted_rows(self.P, self.A, self.Xh))
        return self.main()


@contextlib.contextmanager
def _device_plan(combo, monkeypatch):
    """yields a _Ctx, or None where the planner refuses the combination (the refusal and its message asserted on the
    host and on the device)"""
    import torch
    from neurec_amd import engine as E
    name, d, n_wg, kw = combo
    A = R.case(name)["A"]
    lib = load_plancheck()
    indptr = np.ascontiguousarray(A.indptr, np.int64)
    indices = np.ascontiguousarray(A.indices, np.int32)
    # the switches a plan's creation reads from the environment, set before it
    monkeypatch.setenv("NEUREC_SPMM_MASKED_FAST", str(kw.get("masked_fast", 1)))
    monkeypatch.setenv("NEUREC_SPMM_WANTED_WAVE", str(kw.get("wanted_wave", 1)))
    monkeypatch.delenv("NEUREC_SPMM_PACKED", raising=False)
    if kw.get("wanted_nnz_cap"):
        monkeypatch.setenv("NEUREC_SPMM_WANTED_NNZ_CAP", str(kw["wanted_nnz_cap"]))
    else:
        monkeypatch.delenv("NEUREC_SPMM_WANTED_NNZ_CAP", raising=False)
    P, refusal = None, None
    try:
        args = R.planner_args(build, lib, combo)
        P = build(lib, A, d, n_wg, **args)
    except Refused as e:
        refusal = str(e)
        args = dict(split_row=kw.get("split", 0), **{k: kw[k] for k in ("waves", "seg", "r_max", "p_max") if k in kw})
    assert (refusal is not None) == ("refuse" in kw), (R.combo_id(combo), refusal)
    nbytes = C.c_size_t(0)
    E.call("nrhip_spmm_blocked_plan_bytes", A.shape[0], A.nnz, d, C.byref(nbytes))
    buf = torch.full((max(nbytes.value, 256),), BYTE_CANARY, dtype=torch.uint8, device="cuda")
    _LIVE.append(buf)
    plan = C.c_void_p(0)
    create = lambda: E.call("nrhip_spmm_blocked_plan_create", indptr.ctypes.data_as(C.c_void_p),
                            indices.ctypes.data_as(C.c_void_p), A.shape[0], args.get("split_row", 0), d,
                            args.get("block_bytes", 0), n_wg, args.get("waves", 0), args.get("seg", 0),
                            args.get("r_max", 0), args.get("p_max", 0), _p(buf), buf.numel(), E._stream(), C.byref(plan))
    if refusal is not None:
        with pytest.raises(NotImplementedError) as e:
            create()
        assert kw["refuse"] in refusal and kw["refuse"] in str(e.value) and refusal in str(e.value)
        assert not plan.value
        yield None
        return
    create()
    try:
        info = (C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0))
        E.call("nrhip_spmm_blocked_plan_info", plan, *[C.byref(x) for x in info])
        assert same_plan(_np(buf[:P["used"]]), [x.value for x in info], P) >= 14
        if "phases" in kw:
            assert P["n_phases"] == kw["phases"] or (kw.get("split") and P["n_phases"] > 1)
        ctx = _Ctx(combo, P, plan, buf)
        E.call("nrhip_spmm_blocked_pack", plan, _p(ctx.idx), _p(ctx.val), E._stream())
        if kw.get("gif4"):
            E.call("nrhip_spmm_blocked_tune", 4)
        yield ctx
        torch.cuda.synchronize()
    finally:
        E.call("nrhip_spmm_blocked_plan_destroy", plan)


def _out(n, d):
    """an output buffer: n rows and two more, all canary"""
    import torch
    t = torch.full((n + 2, d), float(CANARY), dtype=torch.float32, device="cuda")
    _LIVE.append(t)
    return t


def _twice(what, run):
    """run() -> tuple of numpy arrays (fresh buffers every time): the same bits twice; returns the first"""
    a, b = run(), run()
    for x, y in zip(a, b):
        if x is not None:
            _bits(y, x, (what, "second run"))
    return a


def _product(ctx, what, Xh=None, want_Y=True, addend=None, sum_in=None, in_place=False, flag=None, xnz=None, wanted=None):
    """nrhip_spmm_blocked(_flagged) on fresh canary buffers, twice; returns (Y, sum_out) as numpy, n + 2 rows each"""
    from neurec_amd import engine as E
    X = _dev(ctx.Xh if Xh is None else Xh)

    def run():
        Y = _out(ctx.n, ctx.d) if want_Y else None
        S_in = S_out = None
        if sum_in is not None:
            S_in = _dev(np.concatenate([sum_in, np.full((2, ctx.d), CANARY, np.float32)]))
            S_out = S_in if in_place else _out(ctx.n, ctx.d)
        Hd = _dev(addend) if addend is not None else None
        common = (_p(S_in), _p(S_out), _p(_dev(xnz)) if xnz is not None else None,
                  _p(_dev(wanted)) if wanted is not None else None, E._stream())
        if flag is not None:
            E.call("nrhip_spmm_blocked_flagged", ctx.plan, _p(ctx.idx), _p(ctx.val), _p(X), _p(Y), _p(Hd), _p(_dev(flag)),
                   *common)
        else:
            E.call("nrhip_spmm_blocked", ctx.plan, _p(ctx.idx), _p(ctx.val), _p(X), _p(Y), _p(Hd), *common)
        return (_np(Y) if want_Y else None, _np(S_out) if S_out is not None else None)
    return _twice((R.combo_id(ctx.combo), what), run)


def _check(ctx, what, got, y, addend=None, sum_in=None, in_place=False, wanted=None, la=None, lb=None):
    """got = (Y, sum_out) of a call; y = the restated rows of A·X"""
    Yw, Sw = R.epilogue(y, addend, sum_in, la, lb)
    if got[0] is not None:
        _bits(got[0], R.keep_canary(Yw, wanted), (R.combo_id(ctx.combo), what, "Y"))
    if sum_in is not None:
        want = R.keep_canary(Sw, wanted)
        if in_place:
            sel = np.zeros(ctx.n, bool) if wanted is None else np.asarray(wanted) == 0
            want[:ctx.n][sel] = sum_in[sel]
        _bits(got[1], want, (R.combo_id(ctx.combo), what, "sum_out"))


def _wanted_masks(ctx):
    rng = _rng(ctx.combo, 2)
    lens = np.diff(ctx.A.indptr)
    masks = {"no row": np.zeros(ctx.n, np.uint8), "every row": np.ones(ctx.n, np.uint8),
             "hub rows": (lens > 64).astype(np.uint8), "short rows": (lens <= 64).astype(np.uint8),
             "5 % of the rows": (rng.rand(ctx.n) < 0.05).astype(np.uint8)}
    masks["5 % of the rows"][ctx.case["hubs"][::2]] = 1            # and every other hub
    return masks


# ================================================================== 1. the full pass
@pytest.mark.parametrize("combo", R.COMBOS, ids=R.combo_id)
def test_full_pass(combo, monkeypatch):
    """spmm_blocked_kernel<plain>: Y, Y + addend, the running sum in place, the sum alone, the addend read by flag —
    every row equals the walk of the plan; a refused combination is refused with the planner's message"""
    from neurec_amd import engine as E
    with _device_plan(combo, monkeypatch) as ctx:
        if ctx is None:
            return
        y = ctx.main()
        H, S = ctx.Hh, ctx.Sh
        _check(ctx, "plain", _product(ctx, "plain"), y)
        _check(ctx, "addend", _product(ctx, "addend", addend=H), y, addend=H)
        _check(ctx, "addend, sum in place", _product(ctx, "in place", addend=H, sum_in=S, in_place=True), y, addend=H,
               sum_in=S, in_place=True)
        _check(ctx, "sum only", _product(ctx, "sum only", want_Y=False, sum_in=S), y, sum_in=S)
        flag = (_rng(combo, 3).rand(ctx.n) < 0.33).astype(np.uint8)
        flag[ctx.case["hubs"][::2]] = 1
        Hn = np.where(flag[:, None] != 0, H, np.float32("nan")).astype(np.float32)
        Hz = np.where(flag[:, None] != 0, H, np.float32(0)).astype(np.float32)
        _check(ctx, "addend by flag", _product(ctx, "flag", addend=Hn, sum_in=S, flag=flag), y, addend=Hz, sum_in=S)
        if ctx.case["factors"] and ctx.n_cols <= ctx.n:
            # the 4-byte packed words, and the two arrays of the same packed plan
            from neurec_amd.graph import factor_values
            rf, cf = (np.ascontiguousarray(f, np.float32) for f in factor_values(ctx.A))
            packed = C.c_int32(0)
            E.call("nrhip_spmm_blocked_pack_factored", ctx.plan, _p(ctx.idx), _p(ctx.val), rf.ctypes.data_as(C.c_void_p),
                   cf.ctypes.data_as(C.c_void_p), ctx.n_cols, E._stream(), C.byref(packed))
            assert packed.value == 1 and E._lib.lib.nrhip_spmm_blocked_is_packed(ctx.plan) == 1
            _check(ctx, "packed words", _product(ctx, "packed", addend=H, sum_in=S), y, addend=H, sum_in=S)
            E.call("nrhip_spmm_blocked_tune_packed", 0)
            _check(ctx, "two arrays of a packed plan", _product(ctx, "unpacked", addend=H, sum_in=S), y, addend=H, sum_in=S)
            E.call("nrhip_spmm_blocked_tune_packed", 1)


# ================================================================== 2. the masked hops
@pytest.mark.parametrize("combo", [c for c in R.COMBOS if "refuse" not in c[3]], ids=R.combo_id)
def test_masked_hops(combo, monkeypatch):
    """the column-masked hop (staged or general, as the plan's switches say), the row-masked hop through the kernel its
    plan reaches (wave-cooperative, staged wanted-rows — chunked where w_nnz_cap binds —, staged masked, general) under
    five `wanted` masks, and both masks together"""
    with _device_plan(combo, monkeypatch) as ctx:
        H, S = ctx.Hh, ctx.Sh
        keep = (_rng(combo, 4).rand(ctx.n_cols) < 0.4).astype(np.uint8)
        Xz = R.zero_rows(ctx.Xh, keep)
        kernel = R.dispatch(ctx.P, "cols")
        _check(ctx, ("cols", kernel), _product(ctx, "cols", Xh=Xz, xnz=keep), ctx.main(keep))
        _check(ctx, ("cols, addend, sum", kernel), _product(ctx, "cols+", Xh=Xz, xnz=keep, addend=H, sum_in=S),
               ctx.main(keep), addend=H, sum_in=S)
        if ctx.n_cols == ctx.n:                                    # an addend that IS the operand shares its promise
            from neurec_amd import engine as E
            Xd, kd, Y = _dev(Xz), _dev(keep), _out(ctx.n, ctx.d)
            E.call("nrhip_spmm_blocked", ctx.plan, _p(ctx.idx), _p(ctx.val), _p(Xd), _p(Y), _p(Xd), None, None, _p(kd),
                   None, E._stream())
            _check(ctx, ("cols, addend = X", kernel), (_np(Y), None), ctx.main(keep), addend=Xz)
        kernel = R.dispatch(ctx.P, "rows")
        for which, wanted in _wanted_masks(ctx).items():
            _check(ctx, ("rows", which, kernel), _product(ctx, which, addend=H, sum_in=S, wanted=wanted), ctx.row_masked(),
                   addend=H, sum_in=S, wanted=wanted)
        wanted = _wanted_masks(ctx)["5 % of the rows"]
        _check(ctx, ("rows, Y alone", kernel), _product(ctx, "rows Y", wanted=wanted), ctx.row_masked(), wanted=wanted)
        kernel = R.dispatch(ctx.P, "both")
        _check(ctx, ("both masks", kernel), _product(ctx, "both", Xh=Xz, xnz=keep, wanted=wanted, addend=H, sum_in=S),
               ctx.main(keep), addend=H, sum_in=S, wanted=wanted)


# ================================================================== 3. the d = 64 hops with their own entries
def _batch(ctx):
    """a batch that names hub rows and repeats rows: (users, pos, neg, n_users)"""
    rng = _rng(ctx.combo, 5)
    n_users = ctx.case["split"] or ctx.n // 2
    hubs = ctx.case["hubs"]
    lo, hi = hubs[hubs < n_users], hubs[hubs >= n_users] - n_users
    b = 24
    users = np.concatenate([lo[:6], rng.randint(0, n_users, b)])[:b]
    pos = np.concatenate([hi[:6], rng.randint(0, ctx.n - n_users, b)])[:b]
    neg = rng.randint(0, ctx.n - n_users, b)
    users[-1], neg[-1], neg[-2] = users[0], neg[0], pos[0]              # repeats, within a list and across lists
    return users.astype(np.int32), pos.astype(np.int32), neg.astype(np.int32), int(n_users)


@pytest.mark.parametrize("combo", ACCEPTED_64, ids=R.combo_id)
def test_wanted_layers_and_batch(combo, monkeypatch):
    """nrhip_spmm_blocked_wanted_layers with and without layer_a / layer_b, nrhip_spmm_blocked_wanted_batch with its
    flags and row list; a plan without the schedule refuses"""
    from neurec_amd import engine as E
    with _device_plan(combo, monkeypatch) as ctx:
        P, S, La, Lb = ctx.P, ctx.Sh, ctx.Lah, ctx.Lbh
        X = _dev(ctx.Xh)
        wanted = _wanted_masks(ctx)["5 % of the rows"]
        kernel = R.dispatch(P, "rows")

        def layers(la, lb):
            def run():
                out = _out(ctx.n, ctx.d)
                E.call("nrhip_spmm_blocked_wanted_layers", ctx.plan, _p(ctx.idx), _p(ctx.val), _p(X), _p(_dev(S)),
                       _p(_dev(la)) if la is not None else None, _p(_dev(lb)) if lb is not None else None, _p(out),
                       _p(_dev(wanted)), E._stream())
                return (None, _np(out))
            return _twice((R.combo_id(combo), "layers"), run)

        if not (P["ww_ok"] or P["wanted_ok"]):
            with pytest.raises(NotImplementedError):
                layers(None, None)
        else:
            for la, lb in ((None, None), (La, None), (La, Lb)):
                _check(ctx, ("layers", la is not None, lb is not None, kernel), layers(la, lb), ctx.row_masked(),
                       sum_in=S, la=la, lb=lb, wanted=wanted)
        users, pos, neg, n_users = _batch(ctx)
        rows = np.concatenate([users, n_users + pos, n_users + neg]).astype(np.int32)
        in_batch = np.zeros(ctx.n, np.uint8)
        in_batch[rows] = 1

        def batch():
            def run():
                import torch
                out = _out(ctx.n, ctx.d)
                flags = _dev(np.concatenate([np.zeros(ctx.n, np.uint8), np.full(2, BYTE_CANARY, np.uint8)]))
                rows_out = _dev(np.full(len(rows) + 2, -77, np.int32))
                E.call("nrhip_spmm_blocked_wanted_batch", ctx.plan, _p(ctx.idx), _p(ctx.val), _p(X), _p(_dev(S)),
                       _p(_dev(La)), _p(_dev(Lb)), _p(out), _p(_dev(users)), _p(_dev(pos)), _p(_dev(neg)), len(users),
                       n_users, _p(flags), _p(rows_out), E._stream())
                return (None, _np(out), _np(flags), _np(rows_out))
            return _twice((R.combo_id(combo), "batch"), run)

        if not (P["ww_ok"] or (P["wanted_ok"] and P["w_bitmap_words"] > 0)):
            with pytest.raises(NotImplementedError):
                batch()
        else:
            got = batch()
            _check(ctx, ("batch", kernel), got[:2], ctx.row_masked(), sum_in=S, la=La, lb=Lb, wanted=in_batch)
            assert np.array_equal(got[2], np.concatenate([in_batch, np.full(2, BYTE_CANARY, np.uint8)]))
            assert np.array_equal(got[3], np.concatenate([rows, np.full(2, -77, np.int32)]))


@pytest.mark.parametrize("combo", ACCEPTED_64, ids=R.combo_id)
def test_adam_pass(combo, monkeypatch):
    """nrhip_spmm_blocked_adam: the tables after the pass equal nrhip_adam_dense_tf (pinned in test_primitives_gpu.py)
    applied to the restated gradient (y + addend) + grad_b, in bits; with clear_consumed the consumed rows and flags
    are zero and the others untouched; a plan of 8 waves refuses"""
    from neurec_amd import engine as E
    with _device_plan(combo, monkeypatch) as ctx:
        rng = _rng(combo, 6)
        n, d = ctx.n, ctx.d
        if ctx.n_cols != n:
            return                                                     # the updated table is the operand's shape: square only
        X = _dev(ctx.Xh)
        H, Gb = ctx.Hh, (rng.randn(n, d) * 0.01).astype(np.float32)
        tail = lambda a, fill=CANARY: np.concatenate([a, np.full((2, d), fill, np.float32)])
        var0, m0, v0 = (tail(a.astype(np.float32)) for a in (rng.randn(n, d), rng.randn(n, d) * 0.01, rng.rand(n, d) * 1e-3))
        st = E.AdamState(0.01)
        st.advance()
        flag = (rng.rand(n) < 0.3).astype(np.uint8)
        flag[ctx.case["hubs"][::2]] = 1
        on = flag[:, None] != 0

        def fused(addend, grad_b, flags):
            def run():
                var, m, v, Hd, Gd = _dev(var0), _dev(m0), _dev(v0), _dev(tail(addend)), _dev(tail(grad_b))
                fl = _dev(np.concatenate([flags, np.full(2, BYTE_CANARY, np.uint8)])) if flags is not None else None
                E.call("nrhip_spmm_blocked_adam", ctx.plan, _p(ctx.idx), _p(ctx.val), _p(X), _p(Hd), _p(Gd), _p(var),
                       _p(m), _p(v), float(st.alpha()), float(st.beta1), float(st.beta2), float(st.eps),
                       1 if flags is not None else 0, _p(fl), E._stream())
                return (_np(var), _np(m), _np(v), _np(Hd), _np(Gd), _np(fl) if fl is not None else None)
            return _twice((R.combo_id(combo), "adam"), run)

        if ctx.P["waves"] != 16:
            with pytest.raises(NotImplementedError):
                fused(H, Gb, None)
            return

        def dense(addend, grad_b):
            g, _ = R.epilogue(R.epilogue(ctx.main(), addend)[0], grad_b)
            var, m, v = _dev(var0), _dev(m0), _dev(v0)
            E.call("nrhip_adam_dense_tf", _p(var), _p(m), _p(v), _p(_dev(g)), n * d, float(st.alpha()), float(st.beta1),
                   float(st.beta2), float(st.eps), 0, E._stream())
            return _np(var), _np(m), _np(v)

        got, want = fused(H, Gb, None), dense(H, Gb)
        for k, name in enumerate(("var", "m", "v")):
            _bits(got[k], want[k], (R.combo_id(combo), "adam", name))
        _bits(got[3], tail(H), "addend left alone")
        _bits(got[4], tail(Gb), "grad_b left alone")
        # clear_consumed with flags: the unflagged rows are promised zero and never read (NaN there)
        nan = np.float32("nan")
        got = fused(np.where(on, H, nan).astype(np.float32), np.where(on, Gb, nan).astype(np.float32), flag)
        want = dense(np.where(on, H, 0).astype(np.float32), np.where(on, Gb, 0).astype(np.float32))
        for k, name in enumerate(("var", "m", "v")):
            _bits(got[k], want[k], (R.combo_id(combo), "adam by flag", name))
        for k in (3, 4):
            assert not got[k][:n][flag != 0].any() and np.isnan(got[k][:n][flag == 0]).all()
            assert (got[k][n:] == CANARY).all()
        assert not got[5][:n].any() and (got[5][n:] == BYTE_CANARY).all()


# ================================================================== 4. the work-item kernels
def _csr(c, **kw):
    from neurec_amd import engine as E
    csr = E.SpmmCSR.from_scipy(c["A"], keep_order=True, **kw)
    csr.lane_group = False
    return csr


@pytest.mark.parametrize("d", [16, 32, 64, 128, 256])
@pytest.mark.parametrize("name,items", [("lengths", (0, 0)), ("lengths", (1, 1)), ("pre", (0, 0)), ("descending", (1, 1)),
                                        ("star", (0, 0)), ("tiny", (0, 0))])
def test_work_item_kernels(name, items, d):
    """nrhip_spmm_csr without a lane-group schedule (spmm_seg_kernel at d < 64, spmm_item_kernel above, spmm_fix_kernel
    for the rows of more than 256 non-zeros), its masked form at d >= 64 and nrhip_spmm_csr_rows with repeated and hub
    rows, with item_rows / item_nnz of 1 and of their defaults, against work_item()"""
    import torch
    c = R.case(name)
    A, n = c["A"], c["A"].shape[0]
    csr = _csr(c, item_rows=items[0], item_nnz=items[1], split_row=c["split"])
    Xh = R.operand(c, d)
    rng = np.random.RandomState(d + n)
    H, S = (rng.randn(n, d).astype(np.float32) for _ in range(2))
    X = _dev(Xh)
    y = R.work_item(A, Xh)
    assert not csr.ensure_schedule(d)

    def run(addend=None, sum_in=None, want_Y=True, xnz=None, wanted=None, Xd=X):
        def once():
            Y, So = _out(n, d) if want_Y else None, _out(n, d) if sum_in is not None else None
            csr.matmul(Xd, out=Y, addend=_dev(addend) if addend is not None else None,
                       sum_in=_dev(sum_in) if sum_in is not None else None, sum_out=So,
                       x_row_nonzero=_dev(xnz) if xnz is not None else None,
                       y_row_wanted=_dev(wanted) if wanted is not None else None)
            return (_np(Y) if want_Y else None, _np(So) if So is not None else None)
        return _twice((name, d, "work item"), once)

    class Where:
        combo, n = (name, d, 0, {"items": items}), A.shape[0]
    _check(Where, "plain", run(), y)
    _check(Where, "addend, sum", run(addend=H, sum_in=S), y, addend=H, sum_in=S)
    _check(Where, "sum only", run(sum_in=S, want_Y=False), y, sum_in=S)
    lens = np.diff(A.indptr)
    if d >= 64:
        keep = (rng.rand(n) < 0.4).astype(np.uint8)
        Xz = R.zero_rows(Xh, keep)
        yz = R.work_item(A, Xz, x_row_nonzero=keep)
        wanted = (rng.rand(n) < 0.1).astype(np.uint8)
        wanted[c["hubs"][::2]] = 1
        _check(Where, "cols", run(xnz=keep, Xd=_dev(Xz), addend=H, sum_in=S), yz, addend=H, sum_in=S)
        _check(Where, "rows", run(wanted=wanted, addend=H, sum_in=S), y, addend=H, sum_in=S, wanted=wanted)
        _check(Where, "both", run(xnz=keep, wanted=wanted, Xd=_dev(Xz)), yz, wanted=wanted)
        # listed rows: hubs, repeats, an empty row
        rows = np.concatenate([c["hubs"][-3:], rng.randint(0, n, 9), np.flatnonzero(lens == 0)[:1]]).astype(np.int32)
        rows = np.concatenate([rows, rows[:2]])
        listed = np.zeros(n, np.uint8)
        listed[rows] = 1

        def listed_once():
            Y, So = _out(n, d), _out(n, d)
            csr.matmul_rows(X, _dev(rows), out=Y, addend=_dev(H), sum_in=_dev(S), sum_out=So)
            return _np(Y), _np(So)
        _check(Where, "listed rows", _twice((name, d, "rows"), listed_once), y, addend=H, sum_in=S, wanted=listed)
    torch.cuda.synchronize()


def test_a_refused_matrix_falls_back_to_the_work_item_kernel():
    """star_wide at d = 256: 53 hub segments in one row, 48 partial slots — the planner refuses on any workgroup count,
    engine.SpmmCSR keeps the work-item kernel, and the bits are work_item()'s (14 segments of 256)"""
    from neurec_amd import engine as E
    c = R.case("star_wide")
    A, n, d = c["A"], c["A"].shape[0], 256
    with pytest.raises(Refused) as e:
        build(load_plancheck(), A, d, 256)
    assert "more than 48 hub segments in one workgroup phase" in str(e.value)
    csr = E.SpmmCSR.from_scipy(A)
    assert not csr.ensure_schedule(d, force=True) and csr.blocked is None
    Xh = R.operand(c, d)
    X = _dev(Xh)

    def once():
        Y = _out(n, d)
        csr.matmul(X, out=Y)
        return (_np(Y), None)

    class Where:
        combo, n = ("star_wide", d, 0, {}), A.shape[0]
    y = R.work_item(A, Xh)
    _check(Where, "fallback", _twice("fallback", once), y)
    assert (y[0].view(np.int32) != R.sequential(A, Xh)[0].view(np.int32)).any()       # the hub's order is observable
