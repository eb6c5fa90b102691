"""The narrow NGCF layer kernels of csrc/dense.hip called directly (nrhip_ngcf_layer_fwd, nrhip_ngcf_layer_bwd,
nrhip_ngcf_workspace_bytes) against tests/ngcf_restatement.py, at 1, 3, 63, 64, 65, 255, 256, 257, 4096, 4097 and 8200
rows (64: the rows of a workgroup and of an MFMA slab; 4096 = 64 slabs: the last size one pass of the reduce loop
serves; 4097 and 8200: its second and third pass) and keep 1.0 and 0.9.  The two row kernels are held to the bits of
the float32 restatement.  The weight gradients (fp32 MFMA per slab, float64 over the slabs) are held to
(64 + 2) 2^-24 sum|terms| per element of the float64 sums over the device's own dT1 / dT2: a slab's partial is at most
64 float32 accumulations, the operand of dW_bi carries one more rounding, the final cast is one.  The output is a
16-column block of a canaried [n + 1][48] buffer, every other output is followed by a canary row, the mask and the
workspace by canaries, and every case runs twice for the same bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import ngcf_restatement as N

pytestmark = pytest.mark.gpu

CANARY = 7.0
BYTE_CANARY = 0xAA
SEED = 2017
D, LD = N.D, 48
WORST = {}              # rows -> (largest weight-gradient error / bound seen, where)

_LIVE = []              # device tensors whose raw addresses a call takes, held until the test ends


@pytest.fixture(autouse=True)
def _hold_device_copies():
    """A call takes raw addresses: an operand built inline must not be freed — and its memory handed to the next
    operand by the caching allocator — before the kernel has run."""
    yield
    del _LIVE[:]


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()                   # a copy: the shared cases are read-only
    _LIVE.append(t)
    return t


def _np(t):
    return t.cpu().numpy()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _call(name, *args):
    from neurec_amd._lib import call
    from neurec_amd.engine import _stream
    call(name, *(args + (_stream(),)))


def _bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), \
        (what, int((got != want).sum()), float(np.abs(got.astype(np.float64) - want).max()) if got.size else 0.0)


def _rows(n, data=None):
    """[n + 1][16] of canaries, contiguous: (whole, the first n rows), holding `data` when given"""
    import torch
    whole = torch.full((n + 1, D), CANARY, device="cuda")
    _LIVE.append(whole)
    if data is not None:
        whole[:n].copy_(_dev(data))
    return whole, whole[:n]


def _block(n, col, data=None):
    """[n + 1][48] of canaries and its block [:n, col : col + 16] (ld = 48: the concatenated Out of two layers)"""
    import torch
    whole = torch.full((n + 1, LD), CANARY, device="cuda")
    _LIVE.append(whole)
    view = whole[:n, col:col + D]
    if data is not None:
        view.copy_(_dev(data))
    assert view.stride(0) == LD and view.data_ptr() % 16 == 0
    return whole, view


def _block_intact(whole, n, col):
    w = _np(whole)
    return bool(np.all(w[:, :col] == CANARY) and np.all(w[:, col + D:] == CANARY) and np.all(w[n:] == CANARY))


def _flat(n, extra, dtype=None, fill=CANARY):
    import torch
    whole = torch.full((n + extra,), fill, device="cuda", dtype=dtype or torch.float32)
    _LIVE.append(whole)
    return whole, whole[:n]


def _tail_intact(whole, n, fill=CANARY):
    return bool(np.all(_np(whole)[n:] == fill))


def _twice(run):
    a, b = run(), run()
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        _bits(x, y, ("repeat", k))
    return a


def _ws_floats(n):
    from neurec_amd._lib import call
    nbytes = C.c_size_t(0)
    call("nrhip_ngcf_workspace_bytes", n, C.byref(nbytes))
    assert nbytes.value % 4 == 0
    return nbytes.value // 4


WEIGHTS = ("Wg", "bg", "Wb", "bb")


def _operands(c):
    """device copies of (ego, S, Wg, bg, Wb, bb) and a check that a call left them as they were"""
    keys = ("ego", "S") + WEIGHTS
    ops = [_dev(c[k]) for k in keys]

    def unchanged():
        for k, t in zip(keys, ops):
            _bits(_np(t), c[k], (k, "unchanged"))
    return ops, unchanged


def _fwd(c, n, keep, mask, col=D, step=3, layer=1):
    """-> (ego_out [n][16], out [n][16], mask bytes [n][16]); mask None: drawn on the device"""
    import torch
    ops, unchanged = _operands(c)
    ew, ego_out = _rows(n)
    ow, out = _block(n, col)
    mw, m = _flat(n * D, 32, torch.uint8, BYTE_CANARY)
    if mask is not None:
        m.copy_(_dev(mask.reshape(-1)))
    _call("nrhip_ngcf_layer_fwd", *[_p(t) for t in ops], n, D, keep, _p(m), int(mask is not None), SEED, step, layer,
          _p(ego_out), _p(out), out.stride(0))
    assert _block_intact(ow, n, col) and np.all(_np(ew)[n:] == CANARY) and _tail_intact(mw, n * D, BYTE_CANARY)
    unchanged()
    return _np(ego_out), _np(out), _np(m).reshape(n, D)


BWD_OUT = ("dS", "d_ego_direct", "dT1", "dT2", "dWg", "dbg", "dWb", "dbb")


def _bwd(c, n, keep, with_next, col=None):
    """-> the eight outputs; col None: d_out contiguous (ld = 16), else the block at `col` of an [n + 1][48] buffer"""
    import torch
    ops, unchanged = _operands(c)
    m = _dev(c["mask"].reshape(-1))
    if col is None:
        gw, g = _rows(n, c["d_out"])
    else:
        gw, g = _block(n, col, c["d_out"])
    g_before = _np(gw)
    nxt = _rows(n, c["d_ego_next"])[1] if with_next else None
    rows = [_rows(n) for _ in range(4)]
    grads = [_flat(k, 8) for k in (D * D, D, D * D, D)]
    ws_n = _ws_floats(n)
    used = -(-n // N.SLAB) * N.SLAB_FLOATS
    assert ws_n >= used
    wsw, ws = _flat(ws_n, 64)
    _call("nrhip_ngcf_layer_bwd", *[_p(t) for t in ops], n, D, keep, _p(m), _p(g), g.stride(0), _p(nxt),
          *[_p(r[1]) for r in rows], *[_p(x[1]) for x in grads], _p(ws), 4 * ws_n)
    for whole, _ in rows:
        assert np.all(_np(whole)[n:] == CANARY)
    for (whole, _), k in zip(grads, (D * D, D, D * D, D)):
        assert _tail_intact(whole, k)
    assert _tail_intact(wsw, used), "the workspace past ceil(n / 64) * 544 floats"
    unchanged()
    _bits(_np(m), c["mask"].reshape(-1), "the mask is only read")
    _bits(_np(gw), g_before, "d_out unchanged")
    return tuple(_np(r[1]) for r in rows) + (_np(grads[0][1]).reshape(D, D), _np(grads[1][1]),
                                              _np(grads[2][1]).reshape(D, D), _np(grads[3][1]))


@functools.lru_cache(maxsize=None)
def _want(n, kind, keep):
    """the float32 restatement of a case, computed once: forward and both backward forms"""
    c = N.layer_inputs(n, kind)
    args = N.layer_args(c)
    pre = N.layer_pre(*args, keep)
    out = {"pre": pre, "fwd": N.layer_fwd(*args, keep, pre=pre)}
    for nx in (False, True):
        out[nx] = N.layer_bwd_rows(*args, keep, c["d_out"], c["d_ego_next"] if nx else None, pre=pre)
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


def _constructed_rows_present(n, kind, keep):
    """the rows the backward must not get wrong are in the case (all of them from 5 rows on, between the two kinds)"""
    c = N.layer_inputs(n, kind)
    T1, T2, z, ss, inv = _want(n, kind, keep)["pre"]
    if n > N.ROW_MASKED:
        assert ss[N.ROW_MASKED] == 0 and c["d_out"][N.ROW_MASKED].any()                      # the zero row
    if kind == "unbiased":
        assert not T1[N.ROW_ZERO_PRE].any() and not T2[N.ROW_ZERO_PRE].any() and c["d_out"][N.ROW_ZERO_PRE].all()
        if n > N.ROW_TINY:
            assert 0 < ss[N.ROW_TINY] < N.NORM_EPS and c["d_out"][N.ROW_TINY].all()         # the tiny-norm row
    if n >= 5:
        assert len(N.zero_dout_rows(n)) >= 1 and not c["d_out"][N.zero_dout_rows(n)].any()
        assert np.all(ss[N.FIRST_PLAIN:] > N.NORM_EPS)


# ================================================================== forward
@pytest.mark.parametrize("n", N.ROWS)
def test_forward_bit_exact(n):
    """ego_out and out against the float32 restatement with the mask given (bytes 2 and 255 count as kept, the mask is
    only read), out the block at column 16 and at column 32 of an [n + 1][48] canary buffer; then with the mask drawn
    on the device: its bytes equal draw_mask16, differ between two steps and two layers, and the outputs equal the
    restatement on that mask.  Idle quads of the last workgroup (every n that is no multiple of 64) store nothing:
    the canary row after row n - 1 of every output stays."""
    for kind in N.KINDS:
        c = N.layer_inputs(n, kind)
        for keep in N.KEEPS:
            want_e, want_o = _want(n, kind, keep)["fwd"]
            for col in (D, 2 * D):
                what = ("fwd", n, kind, keep, col)
                ego, out, m = _twice(lambda: _fwd(c, n, keep, c["mask"], col))
                _bits(ego, want_e, what + ("ego_out",))
                _bits(out, want_o, what + ("out",))
                _bits(m, c["mask"], what + ("a given mask is only read",))
    c = N.layer_inputs(n, "biased")
    for keep in N.KEEPS:
        ego, out, m = _twice(lambda: _fwd(c, n, keep, None, step=3, layer=1))
        drawn = N.draw_mask16(SEED, 3, 1, n, keep)
        _bits(m, drawn, ("drawn mask", n, keep))
        e2, o2 = N.layer_fwd(*N.layer_args(c)[:-1], drawn, keep)
        _bits(ego, e2, ("drawn ego_out", n, keep))
        _bits(out, o2, ("drawn out", n, keep))
        if keep == 1.0:
            assert drawn.all()
        for step, layer in ((4, 1), (3, 2)):
            other = _fwd(c, n, keep, None, step=step, layer=layer)[2]
            _bits(other, N.draw_mask16(SEED, step, layer, n, keep), ("drawn mask", n, keep, step, layer))
            if keep < 1 and n >= 63:
                assert not np.array_equal(other, drawn), (step, layer)


# ================================================================== backward
BWD_FORMS = ((False, None), (True, None), (True, D), (False, 2 * D))       # (d_ego_next given, d_out's column block)


def _check_wgrads(c, n, got, what):
    """the four weight gradients within (64 + 2) 2^-24 sum|terms| of the float64 sums over the device's dT1, dT2"""
    grads, terms = N.layer_wgrads(c["ego"], c["S"], got[2], got[3])
    for name, g, want, t in zip(BWD_OUT[4:], got[4:], grads, terms):
        assert g.dtype == np.float32 and g.shape == want.shape and np.all(np.isfinite(g)), what + (name,)
        err, bound = np.abs(g - want), N.wgrad_bound(t)
        ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0
        if ratio > WORST.get(n, (0.0, ""))[0]:
            WORST[n] = (ratio, what + (name,))
        print("%s %s: largest error / bound %.3g (largest at %d rows so far %.3g at %s)"
              % ((what, name, ratio, n) + WORST.get(n, (0.0, ""))))
        assert np.all(err <= bound), what + (name, float(err.max()), ratio)


@pytest.mark.parametrize("n", N.ROWS)
def test_backward_rows_bit_exact_and_weight_gradients_within_bound(n):
    """dS, d_ego_direct, dT1 and dT2 against the float32 restatement with d_ego_next NULL and given, d_out contiguous
    and a column block of an [n + 1][48] buffer; the cases hold a fully masked row, a row with 0 < ss < 1e-12, a row of
    exactly zero pre-activations (the 0.2 branch) and rows of zero d_out.  Then dW_gc, db_gc, dW_bi and db_bi, from the
    device's own dT1 / dT2 which the first half has held to bits."""
    for kind in N.KINDS:
        c = N.layer_inputs(n, kind)
        for keep in N.KEEPS:
            _constructed_rows_present(n, kind, keep)
            for nx, col in BWD_FORMS:
                what = ("bwd", n, kind, keep, nx, col)
                got = _twice(lambda: _bwd(c, n, keep, nx, col))
                for name, g, want in zip(BWD_OUT[:4], got, _want(n, kind, keep)[nx]):
                    _bits(g, want, what + (name,))
                _check_wgrads(c, n, got, what)


@pytest.mark.parametrize("n,r", [(n, r) for n, rows in sorted(N.MARKER_ROWS.items()) for r in rows])
def test_weight_gradients_of_one_marked_row(n, r):
    """d_out is zero except in row r (entries of size 1, as S[r] and ego[r]), d_ego_next NULL: dT1 and dT2 are zero
    outside row r and every weight gradient is one outer product of that row — a slab, a row of the MFMA's four-row
    load or a pass of the reduce loop that is dropped leaves zeros where the bound allows a few ulp."""
    c = N.marker_inputs(n, r)
    args = N.layer_args(c)
    for keep in N.KEEPS:
        want = N.layer_bwd_rows(*args, keep, c["d_out"], None)
        got = _twice(lambda: _bwd(c, n, keep, False, D))
        for name, g, w in zip(BWD_OUT[:4], got, want):
            _bits(g, w, ("marker", n, r, keep, name))
        dT1, dT2 = (x.astype(np.float64) for x in want[2:])
        others = np.arange(n) != r
        assert not dT1[others].any() and not dT2[others].any() and dT1[r].all() and dT2[r].all()
        bi = (c["ego"][r] * c["S"][r]).astype(np.float64)
        outer = (np.outer(c["S"][r].astype(np.float64), dT1[r]), dT1[r], np.outer(bi, dT2[r]), dT2[r])
        for name, g, w in zip(BWD_OUT[4:], got[4:], outer):
            assert np.all(w != 0) and np.all(np.abs(g - w) <= N.wgrad_bound(np.abs(w))), ("marker", n, r, keep, name)
        _check_wgrads(c, n, got, ("marker", n, r, keep))


# ================================================================== the engine past 4,096 rows
def test_engine_step_past_4096_rows():
    """NGCFEngine on a graph of 2,500 + 1,700 = 4,200 rows (66 slabs: the reduce loop's second pass), masks given: one
    step through the native context and one through the spelled-out launch sequence are bit-equal in every trainable,
    moment and weight gradient, and the weight gradients both leave (the native step does not clear them) lie within
    the same bound of the float64 oracle.train.ngcf_loss_and_grads — sum|terms| from a float64 layer loop over the
    oracle's cache, restated with ngcf_restatement (tied to the oracle in test_ngcf_layer_cpu.py)."""
    import torch
    from neurec_amd.trainer import NGCFEngine
    from oracle import train
    from test_ngcf_gpu import _problem
    F8 = np.float64
    rng, R, A, At, E0, W, U, I = _problem(11, U=2500, I=1700)
    n, B, reg = U + I, 200, 0.01
    assert n == 4200
    native = NGCFEngine(A, At, U, I, E0, W, 0.003, reg, 0.1, 256)
    spelled = NGCFEngine(A, At, U, I, E0, W, 0.003, reg, 0.1, 256)
    assert native._ctx is not None
    spelled._ctx = None
    bu, bp, bn = (rng.randint(0, m, B).astype(np.int32) for m in (U, I, I))
    masks = [(rng.rand(n, D) < 0.9).astype(np.uint8) for _ in W]
    la, lb = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    for eng, loss in ((native, la), (spelled, lb)):
        eng.step(_dev(bu), _dev(bp), _dev(bn), loss, masks=[_dev(m) for m in masks])
    assert torch.equal(la, lb)
    assert torch.equal(native.E0, spelled.E0) and torch.equal(native.mE, spelled.mE) and torch.equal(native.vE, spelled.vE)
    for k in range(len(W)):
        for j in range(4):
            for name in ("W", "mW", "vW", "gW"):
                assert torch.equal(getattr(native, name)[k][j], getattr(spelled, name)[k][j]), (name, k, j)

    keep = float(np.float32(native.keep))                           # what the kernels receive
    A8, At8 = A.astype(F8), At.astype(F8)
    W8 = [tuple(w.astype(F8) for w in ws) for ws in W]
    M8 = [m.astype(F8) for m in masks]
    _, _, wg = train.ngcf_loss_and_grads(A8, At8, E0.astype(F8), W8, M8, keep, U, bu, bp, bn, reg)
    out, cache = train.ngcf_forward(A8, E0.astype(F8), W8, M8, keep)
    iu, ii, ij = bu, U + bp, U + bn
    eu, ei, ej = out[iu], out[ii], out[ij]
    _, g = train.bpr_terms(np.sum(eu * ei, axis=1) - np.sum(eu * ej, axis=1))
    dOut = np.zeros_like(out)
    np.add.at(dOut, iu, g[:, None] * (ei - ej) + reg * eu)
    np.add.at(dOut, ii, g[:, None] * eu + reg * ei)
    np.add.at(dOut, ij, -g[:, None] * eu + reg * ej)
    nxt = None
    for k in range(len(W) - 1, -1, -1):
        ego, S = cache[k][0], cache[k][1]
        Wg, bg, Wb, bb = (w.reshape(-1) if w.shape[0] == 1 else w for w in W8[k])
        dS, dEd, dT1, dT2 = N.layer_bwd_rows(ego, S, Wg, bg, Wb, bb, masks[k], keep, dOut[:, D * (k + 1):D * (k + 2)], nxt)
        _, terms = N.layer_wgrads(ego, S, dT1, dT2)
        nxt = dEd + At8 @ dS
        for j, name in enumerate(BWD_OUT[4:]):
            want, bound = np.asarray(wg[k][j], F8).reshape(terms[j].shape), N.wgrad_bound(terms[j])
            assert np.abs(want).max() > 0 and np.all(bound > 0)
            for which, eng in (("native", native), ("spelled", spelled)):
                got = _np(eng.gW[k][j]).astype(F8).reshape(want.shape)
                ratio = float((np.abs(got - want) / bound).max())
                print("engine, 4200 rows, layer %d %s (%s): largest error / bound %.3g" % (k, name, which, ratio))
                assert ratio <= 1.0, (k, name, which, ratio)


# ================================================================== refusals and empty work
def _canaried_call(n=5):
    """valid operands for both entry points with canary-filled outputs: (fwd(**changes), bwd(**changes), untouched())"""
    import torch
    c = N.layer_inputs(n, "biased")
    ops, unchanged = _operands(c)
    m = _dev(c["mask"].reshape(-1))
    ew, ego_out = _rows(n)
    ow, out = _block(n, D)
    gw, g = _block(n, D, c["d_out"])
    g_before = _np(gw)
    rows = [_rows(n) for _ in range(4)]
    grads = [_flat(k, 8) for k in (D * D, D, D * D, D)]
    ws_n = _ws_floats(n)
    wsw, ws = _flat(ws_n, 64)
    mw, mdraw = _flat(n * D, 32, torch.uint8, BYTE_CANARY)

    def fwd(n_rows=n, d=D, keep=0.9, ldo=LD, null=None, out_ptr=None, given=1):
        ptrs = [_p(t) for t in ops] + [_p(m if given else mdraw), _p(ego_out), out_ptr or _p(out)]
        if null is not None:
            ptrs[null] = None
        _call("nrhip_ngcf_layer_fwd", *ptrs[:6], n_rows, d, keep, ptrs[6], given, SEED, 3, 1, ptrs[7], ptrs[8], ldo)

    def bwd(n_rows=n, d=D, keep=0.9, ldo=LD, null=None, dout_ptr=None, ws_floats=ws_n):
        ptrs = [_p(t) for t in ops] + [_p(m), dout_ptr or _p(g)] + [_p(r[1]) for r in rows] + [_p(x[1]) for x in grads] + [_p(ws)]
        if null is not None:
            ptrs[null] = None
        _call("nrhip_ngcf_layer_bwd", *ptrs[:6], n_rows, d, keep, ptrs[6], ptrs[7], ldo, None, *ptrs[8:17], 4 * ws_floats)

    def untouched():
        assert np.all(_np(ew) == CANARY) and np.all(_np(ow) == CANARY) and np.all(_np(mw) == BYTE_CANARY)
        assert all(np.all(_np(r[0]) == CANARY) for r in rows) and all(np.all(_np(x[0]) == CANARY) for x in grads)
        assert np.all(_np(wsw) == CANARY)
        _bits(_np(gw), g_before, "d_out")
        _bits(_np(m), c["mask"].reshape(-1), "mask")
        unchanged()
    off8 = lambda t: C.c_void_p(t.data_ptr() + 8)                     # 8 bytes into a row: not a float4 address
    return fwd, bwd, untouched, off8(out), off8(g), ws_n


def test_refusals_leave_every_output_alone():
    """Each of these is rejected by the host checks before any launch (nothing here hands a kernel a misaligned or short
    buffer), with the documented error class, and leaves canary-filled outputs, mask and workspace as they were:
    d = 8 / 32 (NotImplementedError); ldo < 16, ldo % 4 != 0, an out / d_out address 8 bytes into a row, keep of 0,
    1.5, -0.5 and NaN — in the backward as well: it divides by keep like the forward —, a negative row count and a NULL
    in each required pointer (ValueError); a workspace one float short (status 4)."""
    from neurec_amd._lib import NeuRecHipError
    fwd, bwd, untouched, out8, g8, ws_n = _canaried_call()
    for name, f, off in (("ngcf_layer_fwd", fwd, {"out_ptr": out8}), ("ngcf_layer_bwd", bwd, {"dout_ptr": g8})):
        for d in (8, 32):
            with pytest.raises(NotImplementedError, match="layer width %d not built" % d):
                f(d=d)
        for changes in ({"ldo": 12}, {"ldo": 15}, {"n_rows": -1}, {"keep": 0.0}, {"keep": 1.5}, {"keep": -0.5},
                        {"keep": float("nan")}, {"keep": float("inf")}):
            with pytest.raises(ValueError, match=name + ": bad arguments"):
                f(**changes)
        for changes in ({"ldo": 50}, {"ldo": 18}, off):
            with pytest.raises(ValueError, match=name + ": .* 16-byte aligned"):
                f(**changes)
        untouched()
    for null in range(9):
        for given in (0, 1):
            with pytest.raises(ValueError, match="ngcf_layer_fwd: bad arguments"):
                fwd(null=null, given=given)
    for null in range(17):
        with pytest.raises(ValueError, match="ngcf_layer_bwd: bad arguments"):
            bwd(null=null)
    with pytest.raises(NeuRecHipError, match="status 4.*workspace too small"):
        bwd(ws_floats=N.SLAB_FLOATS - 1)
    untouched()
    fwd65, bwd65, untouched65, _, _, ws65 = _canaried_call(65)
    with pytest.raises(NeuRecHipError, match="status 4"):
        bwd65(ws_floats=2 * N.SLAB_FLOATS - 1)
    untouched65()


def test_zero_rows_are_a_no_op_and_workspace_bytes():
    from neurec_amd._lib import call
    fwd, bwd, untouched, _, _, ws_n = _canaried_call()
    fwd(n_rows=0)
    fwd(n_rows=0, given=0)
    bwd(n_rows=0)
    untouched()
    for n, slabs in ((0, 0), (1, 1), (64, 1), (65, 2), (4097, 65)):
        assert _ws_floats(n) == (slabs + 1) * N.SLAB_FLOATS, n          # one spare slab: room for zero rows
    assert ws_n == 2 * N.SLAB_FLOATS
    for args in ((5, None), (-1, C.byref(C.c_size_t(0)))):
        with pytest.raises(ValueError, match="ngcf_workspace_bytes"):
            call("nrhip_ngcf_workspace_bytes", *args)
