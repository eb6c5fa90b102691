"""The width-generic dense kernels called directly (csrc/ngcf_wide.hip's row-wise kernels, csrc/vae_wide.hip, the
split-K tail, the 128 x 128 tile and the transpose of csrc/gemm.hip) against tests/dense_restatement.py: bit equality
with the float32 restatement wherever the order of operations is documented and no device libm function is involved,
the float64 restatement within 4 x (float32 restatement's own distance) + 1e-5 max|want| elsewhere (tanhf, expf, logf,
cosf outputs and the float atomics of dwq0_wide), a canary around every strided view and in every row, column or
element a call must leave alone, and every case run twice for the same bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import dense_restatement as R

pytestmark = pytest.mark.gpu

CANARY = 7.0
BYTE_CANARY = 0xAA
WORST = {}              # section -> (largest device err / reference f32 err seen, where)
SEED = 2017


_LIVE = []              # device copies made by _dev, held until the test ends


@pytest.fixture(autouse=True)
def _hold_device_copies():
    """A call takes raw addresses: an operand built inline (_p(_dev(x))) must not be freed — and its memory handed to
    the next operand by the caching allocator — before the kernel has run."""
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
    """the address of a tensor or of a strided view's first element; None stays NULL"""
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


def _within(section, what, got, w32, w64):
    """device err <= 4 x reference f32 err + 1e-5 max|want|, printed as test_primitives_gpu.py prints it"""
    got, w32, w64 = (np.asarray(x, np.float64) for x in (got, w32, w64))
    assert got.shape == w64.shape == w32.shape, (what, got.shape, w32.shape, w64.shape)
    if not got.size:
        return
    err, bar = np.abs(got - w64).max(), np.abs(w32 - w64).max()
    if bar > 0 and err / bar > WORST.get(section, (0.0, ""))[0]:
        WORST[section] = (err / bar, what)
    print("%s: device err %.3g, reference f32 err %.3g (largest ratio of %s so far %.3g at %s)"
          % ((what, err, bar, section) + WORST.get(section, (0.0, ""))))
    assert err <= 4 * bar + 1e-5 * np.abs(w64).max(), (what, err, bar)


def _wide(rows, cols, data=None, before=2, after=3):
    """a [rows][before + cols + after] buffer of canaries and its column block [:, before : before + cols] (row stride
    larger than cols, 8 bytes into the row), holding `data` when given"""
    import torch
    wide = torch.full((rows, before + cols + after), CANARY, device="cuda")
    view = wide[:, before:before + cols]
    if data is not None:
        view.copy_(_dev(np.asarray(data, np.float32)))
    return wide, view


def _intact(wide, cols, before=2):
    w = _np(wide)
    return bool(np.all(w[:, :before] == CANARY) and np.all(w[:, before + cols:] == CANARY))


def _flat(n, extra=8, dtype=None, fill=CANARY):
    """n elements followed by `extra` canaries, contiguous: (whole, the first n)"""
    import torch
    whole = torch.full((n + extra,), fill, device="cuda", dtype=dtype or torch.float32)
    return whole, whole[:n]


def _tail_intact(whole, n, fill=CANARY):
    return bool(np.all(_np(whole)[n:] == fill))


def _twice(run):
    """run() -> tuple of numpy arrays; two runs must give the same bits"""
    a, b = run(), run()
    for x, y in zip(a, b):
        _bits(x, y, "repeat")
    return a


# ================================================================== A. the NGCF row-wise kernels
def _act_fwd(c, n, w, w_pad, keep, mask, given, step=3, layer=1):
    """-> (ego [n][w_pad], out [n][w], mask bytes [n * w]); every output a canaried view"""
    import torch
    T1w, T1 = _wide(n, w, c["T1"])
    T2w, T2 = _wide(n, w, c["T2"])
    ew, ego = _wide(n, w_pad)
    ow, out = _wide(n, w, before=5, after=4)                     # a column block of a concatenated Out
    mwhole, m = _flat(n * w, 16, torch.uint8, BYTE_CANARY)
    if given:
        m.copy_(_dev(mask.reshape(-1)))
    _call("nrhip_ngcf_act_fwd", _p(T1), _p(T2), T1.stride(0), n, w, w_pad, keep, _p(m), int(given), SEED, step, layer,
          _p(ego), ego.stride(0), _p(out), out.stride(0))
    assert _intact(ew, w_pad) and _intact(ow, w, 5) and _tail_intact(mwhole, n * w, BYTE_CANARY)
    assert T1.stride(0) > w and out.stride(0) > w and ego.stride(0) > w_pad
    _bits(_np(T1), c["T1"], "T1 unchanged")
    return _np(ego), _np(out), _np(m)


def _act_bwd(c, n, w, keep, ego, mask, with_next):
    T1w, T1 = _wide(n, w, c["T1"])
    T2w, T2 = _wide(n, w, c["T2"])
    _, d_out = _wide(n, w, c["d_out"], before=5, after=4)
    _, d_next = _wide(n, w, c["d_ego_next"], before=1, after=1)
    _, e = _wide(n, w, ego, before=0, after=2)
    d1w, d1 = _wide(n, w)
    d2w, d2 = _wide(n, w)
    m = _dev(mask.reshape(-1))
    assert d1.stride(0) == T1.stride(0)                          # one ldt serves T1, T2, dT1 and dT2
    _call("nrhip_ngcf_act_bwd", _p(d_out), d_out.stride(0), _p(d_next) if with_next else None, d_next.stride(0), _p(e),
          e.stride(0), _p(T1), _p(T2), T1.stride(0), _p(m), n, w, keep, _p(d1), _p(d2))
    assert _intact(d1w, w) and _intact(d2w, w)
    return _np(d1), _np(d2)


@pytest.mark.parametrize("w", R.NGCF_WIDTHS)
def test_ngcf_act_fwd_and_bwd_bit_exact(w):
    """w x (w_pad = w, _pad(w)) x 1, 3, 4, 5, 1001 rows x keep 1.0, 0.9, every operand a column block (ld > w): with the
    mask given, E' (zero pad columns included), l2_normalize(E'), dT1 and dT2 (d_ego_next NULL and given) are bit-equal
    to the float32 restatement — lane fmaf chains over q, the xor-butterfly wave sum, 1 / sqrtf, ss > 1e-12 both ways
    (an all-zero row, a fully masked row, a row of norm 1e-7).  With the mask drawn, the written bytes equal the Python
    hash restatement, differ between two steps and between two layers, and the outputs equal the restatement on
    that mask."""
    from neurec_amd.ngcf_wide import _pad
    for n in R.NGCF_ROWS:
        c = R.ngcf_inputs(n, w)
        for keep in R.NGCF_KEEPS:
            want_e, want_o = R.ngcf_act_fwd(c["T1"], c["T2"], c["mask"], keep, _pad(w))
            want_b = {nx: R.ngcf_act_bwd(c["d_out"], c["d_ego_next"] if nx else None, want_e[:, :w], c["T1"], c["T2"],
                                         c["mask"], keep) for nx in (False, True)}
            for w_pad in sorted({w, _pad(w)}):
                what = ("act", w, w_pad, n, keep)
                ego, out, m = _twice(lambda: _act_fwd(c, n, w, w_pad, keep, c["mask"], True))
                _bits(ego, want_e[:, :w_pad], what + ("ego",))
                _bits(out, want_o, what + ("out",))
                _bits(m, c["mask"].reshape(-1), what + ("a given mask is only read",))
                for nx in (False, True):
                    d1, d2 = _twice(lambda: _act_bwd(c, n, w, keep, ego[:, :w], c["mask"], nx))
                    _bits(d1, want_b[nx][0], what + ("dT1", nx))
                    _bits(d2, want_b[nx][1], what + ("dT2", nx))
            # drawn masks (the mask does not depend on w_pad)
            ego, out, m = _twice(lambda: _act_fwd(c, n, w, _pad(w), keep, None, False, step=3, layer=1))
            drawn = R.draw_mask(R.layer_mask_key(SEED, 3, 1), n * w, keep)
            _bits(m, drawn, ("drawn mask", w, n, keep))
            e2, o2 = R.ngcf_act_fwd(c["T1"], c["T2"], drawn.reshape(n, w), keep, _pad(w))
            _bits(ego, e2, ("drawn ego", w, n, keep))
            _bits(out, o2, ("drawn out", w, n, keep))
            if keep < 1 and n * w >= 1001:
                assert 0.8 < drawn.mean() < 0.97
                for step, layer in ((4, 1), (3, 2)):
                    other = _act_fwd(c, n, w, _pad(w), keep, None, False, step=step, layer=layer)[2]
                    _bits(other, R.draw_mask(R.layer_mask_key(SEED, step, layer), n * w, keep), ("mask", step, layer))
                    assert not np.array_equal(other, drawn), (step, layer)
            if keep == 1.0:
                assert drawn.all()


@pytest.mark.parametrize("w", R.NGCF_WIDTHS)
def test_ngcf_mix_bwd_and_ew_mul_bit_exact(w):
    """dS = Y1 + Y2 * ego (two roundings), d_ego_direct = Y2 * S, pad columns w .. w_pad - 1 zeroed, the row padding
    beyond w_pad untouched; ew_mul with three different leading dimensions"""
    from neurec_amd.ngcf_wide import _pad
    for n in R.NGCF_ROWS:
        c = R.ngcf_inputs(n, w)
        for w_pad in sorted({w, _pad(w)}):
            want = R.ngcf_mix_bwd(c["Y1"], c["Y2"], c["ego"], c["S"], w_pad)

            def run():
                _, Y1 = _wide(n, w, c["Y1"])
                _, Y2 = _wide(n, w, c["Y2"])
                ego = np.full((n, w_pad), CANARY, np.float32)         # the pad columns of the inputs are not read
                S = ego.copy()
                ego[:, :w], S[:, :w] = c["ego"], c["S"]
                _, e = _wide(n, w_pad, ego, before=1, after=2)
                _, s = _wide(n, w_pad, S, before=1, after=2)
                dsw, ds = _wide(n, w_pad, before=1, after=2)          # one lde serves ego, S, dS and d_ego_direct
                dew, de = _wide(n, w_pad, before=1, after=2)
                _call("nrhip_ngcf_mix_bwd", _p(Y1), _p(Y2), Y1.stride(0), _p(e), _p(s), e.stride(0), n, w, w_pad, _p(ds),
                      _p(de))
                assert _intact(dsw, w_pad, 1) and _intact(dew, w_pad, 1)
                return _np(ds), _np(de)
            ds, de = _twice(run)
            _bits(ds, want[0], ("mix dS", w, w_pad, n))
            _bits(de, want[1], ("mix d_ego", w, w_pad, n))

        def mul():
            _, a = _wide(n, w, c["Y1"], before=0, after=1)
            _, b = _wide(n, w, c["Y2"], before=2, after=3)
            ow, o = _wide(n, w, before=4, after=5)
            assert len({a.stride(0), b.stride(0), o.stride(0)}) == 3
            _call("nrhip_ew_mul", _p(a), a.stride(0), _p(b), b.stride(0), n, w, _p(o), o.stride(0))
            assert _intact(ow, w, 4)
            return (_np(o),)
        _bits(_twice(mul)[0], R.ew_mul(c["Y1"], c["Y2"]), ("ew_mul", w, n))


def _drop_fwd(c, n, w, w_pad, keep, flags, mask, given, outs, step=3, layer=1, hand_mask=None):
    """hand_mask: whether the mask buffer is handed over (default: only with the dropout flag, else NULL)"""
    import torch
    hand_mask = bool(flags & 2) if hand_mask is None else hand_mask
    Tw, T = _wide(n, w, c["T1"])
    aw, a = _wide(n, w_pad, before=1, after=2)
    bw, b = _wide(n, w, before=5, after=4)
    mwhole, m = _flat(n * w, 16, torch.uint8, BYTE_CANARY)
    if given and mask is not None:
        m.copy_(_dev(mask.reshape(-1)))
    _call("nrhip_lrelu_drop_fwd", _p(T), T.stride(0), n, w, w_pad, keep, _p(m) if hand_mask else None, int(given), SEED,
          step, layer, flags, _p(a) if "a" in outs else None, a.stride(0), _p(b) if "b" in outs else None, b.stride(0))
    assert _intact(aw, w_pad, 1) and _intact(bw, w, 5) and _tail_intact(mwhole, n * w, BYTE_CANARY)
    return _np(a), _np(b), _np(m)


@pytest.mark.parametrize("w", R.NGCF_WIDTHS)
def test_lrelu_drop_fwd_and_bwd_bit_exact(w):
    """w_pad = w and _pad(w) x flags 0 .. 3 (1: leaky_relu, 2: dropout) x out_a only / out_b only / both x mask given /
    drawn: out_a holds the row with zero pad columns w .. w_pad - 1 (none when w_pad = w), out_b the w real columns
    and nothing beyond, an output not asked for keeps
    its canary; the drawn mask equals the hash restatement and differs between layers and steps.  Backward: d_b NULL
    and given."""
    from neurec_amd.ngcf_wide import _pad
    untouched = lambda n, k: np.full((n, k), CANARY, np.float32)
    for n in R.NGCF_ROWS:
        c = R.ngcf_inputs(n, w)
        for keep in R.NGCF_KEEPS:
            for flags in (0, 1, 2, 3):
                if keep == 1.0 and not flags & 2 and n != 5:
                    continue                                      # keep is not read without the dropout flag
                want = R.lrelu_drop_fwd(c["T1"], c["mask"], keep, flags)
                for w_pad in sorted({w, _pad(w)}):                # w_pad = w: out_a has no pad columns, like out_b
                    padded = np.zeros((n, w_pad), np.float32)
                    padded[:, :w] = want
                    assert padded.shape[1] == w or not padded[:, w:].any()
                    for outs in ("a", "b", "ab"):
                        a, b, m = _twice(lambda: _drop_fwd(c, n, w, w_pad, keep, flags, c["mask"], True, outs))
                        what = ("lrelu_drop_fwd", w, w_pad, n, keep, flags, outs)
                        _bits(a, padded if "a" in outs else untouched(n, w_pad), what + ("out_a",))
                        _bits(b, want if "b" in outs else untouched(n, w), what + ("out_b",))
                        if flags & 2:
                            _bits(m, c["mask"].reshape(-1), what + ("mask",))
                    if flags & 2:
                        a, b, m = _twice(lambda: _drop_fwd(c, n, w, w_pad, keep, flags, None, False, "ab", step=5, layer=2))
                        drawn = R.draw_mask(R.layer_mask_key(SEED, 5, 2), n * w, keep)
                        _bits(m, drawn, ("lrelu_drop drawn mask", w, w_pad, n, keep))
                        _bits(b, R.lrelu_drop_fwd(c["T1"], drawn.reshape(n, w), keep, flags),
                              ("lrelu_drop drawn", w, w_pad, n, keep))
                        _bits(a[:, :w], b, "out_a and out_b agree")
                        assert not a[:, w:].any()
                        if keep < 1 and n * w >= 1001 and w_pad == _pad(w):
                            for step, layer in ((6, 2), (5, 3)):
                                other = _drop_fwd(c, n, w, w_pad, keep, flags, None, False, "b", step=step, layer=layer)[2]
                                assert not np.array_equal(other, drawn), (step, layer)
                    else:             # no dropout: a mask buffer handed over is neither read nor drawn into; NULL is accepted
                        a, b, m = _drop_fwd(c, n, w, w_pad, keep, flags, None, False, "ab", hand_mask=True)
                        assert np.all(m == BYTE_CANARY)
                        _bits(b, want, ("lrelu_drop_fwd with an unused mask buffer", w, w_pad, n, flags))
                        _bits(_drop_fwd(c, n, w, w_pad, keep, flags, None, False, "b")[1], want, "NULL mask")
                for with_b in (False, True):
                    def bwd():
                        _, da = _wide(n, w, c["d_a"], before=1, after=2)
                        _, db = _wide(n, w, c["d_b"], before=5, after=4)
                        _, T = _wide(n, w, c["T1"])
                        whole, dT = _flat(n * w)
                        _call("nrhip_lrelu_drop_bwd", _p(da), da.stride(0), _p(db) if with_b else None, db.stride(0),
                              _p(T) if flags & 1 else None, T.stride(0), _p(_dev(c["mask"].reshape(-1))) if flags & 2 else None,
                              n, w, keep, flags, _p(dT))
                        assert _tail_intact(whole, n * w)
                        return (_np(dT).reshape(n, w),)
                    _bits(_twice(bwd)[0], R.lrelu_drop_bwd(c["d_a"], c["d_b"] if with_b else None, c["T1"], c["mask"], keep,
                                                          flags), ("lrelu_drop_bwd", w, n, keep, flags, with_b))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_edge_dropout_and_gather_f32(n):
    """edge_dropout: out = kept ? vals * (1 / keep) : 0 with the keep bytes given and drawn (key seed ^ (step * golden +
    0x6e6f6465): different from every layer's mask), keep 1.0 and 0.9; gather_f32 with repeated and reversed indices"""
    import torch
    rs = np.random.RandomState(n)
    vals = rs.randn(n).astype(np.float32)
    given = (rs.rand(n) < 0.9).astype(np.uint8)
    for keep in R.NGCF_KEEPS:
        for use_given in (True, False):
            def run(step=9):
                kwhole, k = _flat(n, 16, torch.uint8, BYTE_CANARY)
                if use_given:
                    k.copy_(_dev(given))
                owhole, o = _flat(n)
                _call("nrhip_edge_dropout", _p(_dev(vals)), n, keep, _p(k), int(use_given), SEED, step, _p(o))
                assert _tail_intact(kwhole, n, BYTE_CANARY) and _tail_intact(owhole, n)
                return _np(o), _np(k)
            out, kept = _twice(run)
            want_k = given if use_given else R.draw_mask(R.edge_mask_key(SEED, 9), n, keep)
            _bits(kept, want_k, ("edge_dropout kept", n, keep, use_given))
            _bits(out, R.edge_dropout(vals, want_k, keep), ("edge_dropout", n, keep, use_given))
            if not use_given and keep < 1 and n >= 255:
                assert not np.array_equal(run(step=10)[1], kept)
                assert not np.array_equal(R.draw_mask(R.layer_mask_key(SEED, 9, 0), n, keep), kept)
    src = rs.randn(300).astype(np.float32)
    half = min(n // 2, 300)
    idx = np.r_[np.arange(300)[::-1][:half], rs.randint(0, 300, n - half)].astype(np.int32)   # reversed, then repeats
    assert len(idx) == n and idx.min() >= 0 and idx.max() < len(src)

    def gather():
        whole, dst = _flat(n)
        _call("nrhip_gather_f32", _p(_dev(src)), _p(_dev(idx)), n, _p(dst))
        assert _tail_intact(whole, n)
        return (_np(dst),)
    _bits(_twice(gather)[0], src[idx], ("gather_f32", n))
    assert n < 255 or len(np.unique(idx)) < n


def test_ngcf_rowwise_refusals_and_empty_work():
    """w = 0, w = 257, w_pad < w and keep = 0 are refused as bad arguments and write nothing; n_rows = 0 (and n = 0)
    returns OK with the NULL pointers of empty tensors — an empty device tensor has no storage"""
    import torch
    c = R.ngcf_inputs(4, 24)
    T1w, T1 = _wide(4, 24, c["T1"])
    T2w, T2 = _wide(4, 24, c["T2"])
    ew, ego = _wide(4, 32)
    ow, out = _wide(4, 24)
    m = torch.full((4 * 24,), BYTE_CANARY, dtype=torch.uint8, device="cuda")
    fwd = lambda n, w, w_pad, keep: _call("nrhip_ngcf_act_fwd", _p(T1), _p(T2), 300, n, w, w_pad, keep, _p(m), 0, SEED, 1,
                                          0, _p(ego), 300, _p(out), 300)
    bwd = lambda n, w, keep: _call("nrhip_ngcf_act_bwd", _p(out), 300, None, 0, _p(ego), 300, _p(T1), _p(T2), 300, _p(m), n,
                                   w, keep, _p(ego), _p(out))
    for w, w_pad, keep in ((0, 16, 0.9), (257, 257, 0.9), (24, 16, 0.9), (24, 32, 0.0)):
        with pytest.raises(ValueError, match="ngcf_act_fwd"):
            fwd(4, w, w_pad, keep)
    for w, keep in ((0, 0.9), (257, 0.9), (24, 0.0)):
        with pytest.raises(ValueError, match="ngcf_act_bwd"):
            bwd(4, w, keep)
    with pytest.raises(ValueError, match="lrelu_drop_fwd"):
        _call("nrhip_lrelu_drop_fwd", _p(T1), 29, 4, 24, 16, 0.9, _p(m), 0, SEED, 1, 0, 3, _p(ego), 37, None, 0)
    with pytest.raises(ValueError, match="edge_dropout"):
        _call("nrhip_edge_dropout", _p(T1), 4, 0.0, _p(m), 0, SEED, 1, _p(out))
    fwd(0, 24, 32, 0.9)
    bwd(0, 24, 0.9)
    empty_f, empty_b, empty_i = (torch.empty(0, dtype=d, device="cuda") for d in (torch.float32, torch.uint8, torch.int32))
    assert empty_f.data_ptr() == 0
    z = _p(empty_f) if empty_f.data_ptr() else None
    _call("nrhip_ngcf_act_fwd", z, z, 24, 0, 24, 32, 0.9, None, 0, SEED, 1, 0, z, 32, z, 24)
    _call("nrhip_ngcf_act_bwd", z, 24, None, 0, z, 24, z, z, 24, None, 0, 24, 0.9, z, z)
    _call("nrhip_ngcf_mix_bwd", z, z, 24, z, z, 32, 0, 24, 32, z, z)
    _call("nrhip_ew_mul", z, 24, z, 24, 0, 24, z, 24)
    _call("nrhip_lrelu_drop_fwd", z, 24, 0, 24, 32, 0.9, None, 0, SEED, 1, 0, 3, z, 32, z, 24)
    _call("nrhip_lrelu_drop_bwd", z, 24, None, 0, z, 24, None, 0, 24, 0.9, 3, z)
    _call("nrhip_edge_dropout", z, 0, 0.9, None, 0, SEED, 1, z)
    _call("nrhip_gather_f32", z, None, 0, z)
    for wide, cols in ((T1w, 24), (T2w, 24), (ew, 32), (ow, 24)):
        assert _intact(wide, cols)
    _bits(_np(T1), c["T1"], "T1")
    assert np.all(_np(ego) == CANARY) and np.all(_np(out) == CANARY) and np.all(_np(m) == BYTE_CANARY)
    with pytest.raises(ValueError, match="ngcf_act_fwd"):          # work with a NULL operand is still refused
        _call("nrhip_ngcf_act_fwd", None, _p(T2), 29, 4, 24, 32, 0.9, _p(m), 0, SEED, 1, 0, _p(ego), 37, _p(out), 29)


# ================================================================== B. the Mult-VAE wide kernels
BAG_WIDTHS = (1, 63, 64, 65, 256, 257, 600)


def _bag_call(width, W, bias, act, keep, drop, step, with_h0=True):
    indptr, indices, rows = R.bag_csr()
    hwhole, h0 = _flat(len(indices))
    ywhole, Y = _flat(len(rows) * width)
    _call("nrhip_vae_bag_fwd", _p(_dev(indptr)), _p(_dev(indices)), _p(_dev(rows)), len(rows), width, _p(_dev(W)),
          _p(_dev(bias)), act, keep, None if drop is None else _p(_dev(drop)), SEED, step, _p(h0) if with_h0 else None, _p(Y))
    assert _tail_intact(hwhole, len(indices)) and _tail_intact(ywhole, len(rows) * width)
    return _np(Y).reshape(len(rows), width), _np(h0)


@pytest.mark.parametrize("width", BAG_WIDTHS)
def test_vae_bag_fwd(width):
    """10 batch rows over a 24-user CSR — 0, 1, 7, 8, 9, 63, 64, 65 and 129 items (both sides of the 8-gather walk and
    of the 64-entry deal, a third deal of one entry), non-adjacent users, one user twice — x activation -1, 0 .. 3 x
    dropout given at keep 0.8, drawn at keep 0.8, keep 1.0: h0val holds (1 / sqrt(n)) / keep * mask bit for bit at
    exactly the batch's CSR positions (canary elsewhere); the drawn mask is the hash restatement's; Y before the
    activation is the ascending-item fmaf chain plus the bias bit for bit (relu and identity stay bit-equal); tanh and
    sigmoid are held by the 4 x rule; h0val = NULL is accepted"""
    indptr, indices, rows = R.bag_csr()
    rs = np.random.RandomState(width)
    W, bias = rs.randn(R.BAG_ITEMS, width).astype(np.float32), rs.randn(width).astype(np.float32)
    given = (rs.rand(len(indices)) < 0.8).astype(np.float32)
    for mode, keep, drop, kept in (("given", 0.8, given, given),
                                   ("drawn", 0.8, None, R.draw_bag_keep(R.bag_drop_key(SEED, 4), len(indices), 0.8)),
                                   ("keep 1", 1.0, None, np.ones(len(indices), np.float32))):
        pos, vals, pre32, _ = R.vae_bag_fwd(indptr, indices, rows, W, bias, -1, keep, kept)
        pre64 = R.vae_bag_fwd(indptr, indices, rows, W.astype(np.float64), bias.astype(np.float64), -1, keep, kept)[2]
        want_h = np.full(len(indices), CANARY, np.float32)
        want_h[pos] = vals
        if mode == "drawn":
            assert 0 < kept[pos].sum() < len(pos)
            other = _bag_call(width, W, bias, -1, keep, None, 5)[1]                   # another step: another mask
            assert not np.array_equal(other, want_h) and np.array_equal(other == CANARY, want_h == CANARY)
        for act in (-1, 0, 1, 2, 3):
            Y, h0 = _twice(lambda: _bag_call(width, W, bias, act, keep, drop, 4))
            what = "bag_fwd width=%d %s act=%d" % (width, mode, act)
            _bits(h0, want_h, what + " h0val")
            if act in (0, 1):
                _within("bag_fwd", what, Y, R.act_fwd(act, pre32), R.act_fwd(act, pre64))
            else:
                _bits(Y, R.act_fwd(act, pre32), what)
        Y, h0 = _bag_call(width, W, bias, -1, keep, drop, 4, with_h0=False)
        _bits(Y, pre32, "h0val = NULL")
        assert np.all(h0 == CANARY)


@pytest.mark.parametrize("z", [1, 12, 63, 64, 65, 200])
def test_vae_sample_and_its_backward(z):
    """batch 1, 3, 4, 5, 130 (four rows share a block) x is_training 0, 1 with eps given: EPSSTD, ZS and KLb within the
    4 x rule (expf); eps drawn: repeatable for one (seed, step), different for another step, and EPSSTD / exp(logvar /
    2) within the rule of the Box-Muller draw restated in float64 (logf, cosf).  vae_sample_bwd at anneal 0 and 0.2."""
    for batch in (1, 3, 4, 5, 130):
        rs = np.random.RandomState(1000 * z + batch)
        H2 = (0.5 * rs.randn(batch, 2 * z)).astype(np.float32)
        eps = (0.01 * rs.randn(batch, z)).astype(np.float32)
        dZ = rs.randn(batch, z).astype(np.float32)

        def sample(training, given, step=2):
            ew, e = _flat(batch * z)
            zw, zs = _flat(batch * z)
            kw, kl = _flat(batch)
            _call("nrhip_vae_sample", _p(_dev(H2)), batch, z, _p(_dev(eps)) if given else None, training, SEED, step, _p(e),
                  _p(zs), _p(kl))
            assert _tail_intact(ew, batch * z) and _tail_intact(zw, batch * z) and _tail_intact(kw, batch)
            return _np(e).reshape(batch, z), _np(zs).reshape(batch, z), _np(kl)
        for training in (0.0, 1.0):
            got = _twice(lambda: sample(training, True))
            w32 = R.vae_sample(H2, eps, training)
            w64 = R.vae_sample(H2.astype(np.float64), eps.astype(np.float64), training)
            for name, g, a, b in zip(("EPSSTD", "ZS", "KLb"), got, w32, w64):
                _within("vae_sample", "vae_sample z=%d B=%d training=%g %s" % (z, batch, training, name), g, a, b)
            if training == 0.0:
                _bits(got[1], H2[:, :z], "ZS = mu outside training")
        drawn = _twice(lambda: sample(1.0, False))[0]
        sd64 = np.exp(0.5 * H2[:, z:].astype(np.float64))
        _within("vae_sample", "vae_sample z=%d B=%d drawn eps" % (z, batch), drawn.astype(np.float64) / sd64,
                R.draw_eps(SEED, 2, batch, z, np.float32), R.draw_eps(SEED, 2, batch, z, np.float64))
        assert not np.array_equal(sample(1.0, False, step=3)[0], drawn)
        es = R.vae_sample(H2, eps, 1.0)[0]
        for anneal in (0.0, 0.2):
            def bwd():
                whole, dH2 = _flat(batch * 2 * z)
                _call("nrhip_vae_sample_bwd", _p(_dev(dZ)), _p(_dev(H2)), _p(_dev(es)), batch, z, anneal, _p(dH2))
                assert _tail_intact(whole, batch * 2 * z)
                return (_np(dH2).reshape(batch, 2 * z),)
            got = _twice(bwd)[0]
            f = lambda a: a.astype(np.float64)
            _within("vae_sample_bwd", "vae_sample_bwd z=%d B=%d anneal=%g" % (z, batch, anneal), got,
                    R.vae_sample_bwd(dZ, H2, es, anneal), R.vae_sample_bwd(f(dZ), f(H2), f(es), anneal))
            if anneal == 0.0:                                     # no expf term left: the documented order, bit for bit
                _bits(got, R.vae_sample_bwd(dZ, H2, es, 0.0), "vae_sample_bwd anneal=0")


@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_act_bwd_bit_exact(n):
    """dA = dY * act'(Y) for tanh (1 - y y), sigmoid (y (1 - y)), relu and identity, out of place and in place (dA is
    dY, as neurec_amd/vae_wide.py calls it)"""
    rs = np.random.RandomState(n % 1000)
    dY = rs.randn(n).astype(np.float32)
    for act in range(4):
        Y = R.act_fwd(act, rs.randn(n).astype(np.float32))
        Y[::7] = 0
        want = R.act_bwd(act, dY, Y)
        d_dY, d_Y = _dev(dY), _dev(Y)

        def out_of_place():
            whole, dA = _flat(n)
            _call("nrhip_act_bwd", _p(d_dY), _p(d_Y), n, act, _p(dA))
            assert _tail_intact(whole, n)
            return (_np(dA),)

        def in_place():
            whole, io = _flat(n)
            io.copy_(d_dY)
            _call("nrhip_act_bwd", _p(io), _p(d_Y), n, act, _p(io))
            assert _tail_intact(whole, n)
            return (_np(io),)
        _bits(_twice(out_of_place)[0], want, ("act_bwd", n, act))
        _bits(_np(d_dY), dY, "dY unchanged")
        _bits(_twice(in_place)[0], want, ("act_bwd in place", n, act))
        _bits(_np(d_Y), Y, "Y unchanged")


@pytest.mark.parametrize("cols", [1, 700, 1024, 1025, 2500])
def test_vae_softmax_dlogits(cols):
    """five rows with 0, 1, 1023, 1024 and 1025 items (as many as cols allows) and a logit near 80 in each (95 in one:
    without the max shift expf overflows), a sixth of ordinary logits (|x| <= 3) with 37 items, ld = cols padded to 64:
    nll and the in-place slab within the 4 x rule, the slab row by row — beside a logit of 80 a row's softmax is
    one-hot and 1e-5 of its largest entry would hide every other column of the batch — the pad columns unchanged, a
    row without items all-zero"""
    S, items, ld = R.softmax_case(cols)
    order = np.array([3, 0, 5, 4, 1, 2])                               # batch row r is user order[r]
    counts = [len(i) for i in items]
    indptr = np.r_[0, np.cumsum(counts)].astype(np.int64)
    indices = np.concatenate(items).astype(np.int32) if sum(counts) else np.zeros(1, np.int32)
    Sb = S[order]
    its = [items[u] for u in order]

    def run():
        slab = _dev(Sb)
        whole, nll = _flat(6)
        _call("nrhip_vae_softmax_dlogits", _p(slab), ld, 6, cols, _p(_dev(indptr)), _p(_dev(indices)),
              _p(_dev(order.astype(np.int32))), _p(nll))
        assert _tail_intact(whole, 6)
        return _np(nll), _np(slab)
    nll, slab = _twice(run)
    n32, d32 = R.softmax_dlogits(Sb[:, :cols], its)
    n64, d64 = R.softmax_dlogits(Sb[:, :cols].astype(np.float64), its)
    _within("softmax", "softmax_dlogits cols=%d nll" % cols, nll, n32, n64)
    for r in range(6):
        _within("softmax", "softmax_dlogits cols=%d dlogits of row %d (%d items)" % (cols, r, len(its[r])),
                slab[r, :cols], d32[r], d64[r])
    _bits(slab[:, cols:], Sb[:, cols:], "pad columns")
    assert np.isfinite(nll).all() and not slab[1, :cols].any() and counts[order[1]] == 0


@pytest.mark.parametrize("width", [1, 64, 65, 300])
def test_vae_dwq0_wide(width):
    """dW_q0[item] += h0val[t] * dA1[b] over the batch's CSR positions (batch rows share items; one user is named
    twice): exact whatever order the atomics take on dyadic values (multiples of 1/4: every product and partial sum is
    exact in float32), within the 4 x rule on random ones; item rows named by no batch entry stay untouched"""
    indptr, indices, rows = R.bag_csr()
    rs = np.random.RandomState(width)
    named = np.unique(np.concatenate([indices[indptr[u]:indptr[u + 1]] for u in rows]))
    still = np.setdiff1d(np.arange(R.BAG_ITEMS), named)
    assert len(still) and len(named) > 100
    for dyadic in (True, False):
        if dyadic:
            h0, DA1, dW = (rs.randint(-7, 8, s) / 4.0 for s in (len(indices), (len(rows), width), (R.BAG_ITEMS, width)))
        else:
            h0, DA1, dW = rs.randn(len(indices)), rs.randn(len(rows), width), rs.randn(R.BAG_ITEMS, width)
        h0, DA1, dW = (a.astype(np.float32) for a in (h0, DA1, dW))

        def run():
            whole, out = _flat(R.BAG_ITEMS * width)
            out.copy_(_dev(dW.reshape(-1)))
            _call("nrhip_vae_dwq0_wide", _p(_dev(indptr)), _p(_dev(indices)), _p(_dev(rows)), len(rows), width,
                  _p(_dev(h0)), _p(_dev(DA1)), _p(out))
            assert _tail_intact(whole, R.BAG_ITEMS * width)
            return (_np(out).reshape(R.BAG_ITEMS, width),)
        got = _twice(run)[0] if dyadic else run()[0]           # exact sums repeat; the order of the atomics need not
        w32 = R.dwq0_wide(indptr, indices, rows, h0, DA1, dW.copy())
        if dyadic:
            _bits(got, w32, ("dwq0 dyadic", width))
        else:
            f = lambda a: a.astype(np.float64)
            _within("dwq0_wide", "dwq0_wide width=%d" % width, got, w32, R.dwq0_wide(indptr, indices, rows, f(h0), f(DA1), f(dW)))
        _bits(got[still], dW[still], ("dwq0 unnamed item rows", width))
        assert not np.array_equal(got[named], dW[named])


COLSUM_ROWS = (0, 1, 15, 16, 17, 511, 512, 513, 2048, 2049, 2561)


def _colsum(X, rows, cols, ws_floats):
    """-> (out with its canary tail, status).  ws_floats: size of the workspace handed over (None: no workspace)"""
    from neurec_amd._lib import NeuRecHipError
    _, x = _wide(max(rows, 1), cols, X if rows else None)
    whole, out = _flat(cols)
    wsw = ws = None
    if ws_floats is not None:
        wsw, ws = _flat(ws_floats)
    try:
        _call("nrhip_colsum_rows", _p(x) if rows else None, x.stride(0), rows, cols, _p(out), _p(ws),
              0 if ws is None else 4 * ws_floats)
        status = 0
    except NeuRecHipError as e:
        status = int(str(e).split("status ")[1].split(":")[0])
    assert wsw is None or _tail_intact(wsw, ws_floats)
    assert status == 0 or wsw is None or np.all(_np(wsw) == CANARY)          # a refused call wrote nothing there either
    return _np(whole), status


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 300])
def test_colsum_rows(cols):
    """rows 0, 1, 15, 16, 17 (the 16 row groups), 511 .. 513, 2,048 (the last single-block size) and 2,049, 2,561 (512-row
    chunks, a second level, the last chunk of 1 row) with ld > cols: bit-equal to the float32 restatement (16 group
    sums in row order, added in group order, chunk sums likewise) and within the 4 x rule of float64; rows = 0 writes
    zeros (X may be NULL); above 2,048 rows a missing workspace, or one a float short, is refused with the workspace
    status and nothing is written; a workspace of exactly ceil(rows / 512) * cols floats is enough and nothing is
    written beyond it"""
    from neurec_amd._lib import ERR_WORKSPACE
    rs = np.random.RandomState(cols)
    for rows in COLSUM_ROWS:
        X = rs.randn(rows, cols).astype(np.float32)
        need = -(-rows // 512) * cols if rows > 2048 else None
        got, status = _colsum(X, rows, cols, need)
        _bits(_colsum(X, rows, cols, need)[0], got, "repeat")
        assert status == 0 and np.all(got[cols:] == CANARY)
        w32 = R.colsum_rows(X)
        _bits(got[:cols], w32, ("colsum_rows", rows, cols))
        _within("colsum_rows", "colsum_rows rows=%d cols=%d" % (rows, cols), got[:cols], w32, R.colsum_rows(X.astype(np.float64)))
        if rows == 0:
            assert not got[:cols].any()
        if rows > 2048:
            for short in (None, need - 1):
                got, status = _colsum(X, rows, cols, short)
                assert status == ERR_WORKSPACE and np.all(got == CANARY), (rows, cols, short, status)


def test_vae_wide_batch_limit_and_empty_work():
    """vae_bag_fwd and vae_dwq0_wide launch one grid row per batch row: batch = 65,536 is refused up front as
    unsupported (nothing is launched, nothing written); batch = 0, n = 0 and rows = 0 return OK with the NULL pointers
    of empty tensors; a GEMM with K = 0 takes NULL A and B and leaves C (+)= 0 with the epilogue"""
    indptr, indices, rows = R.bag_csr()
    d_ip, d_ix, d_rows = _dev(indptr), _dev(indices), _dev(rows)
    W, bias = _dev(np.ones((R.BAG_ITEMS, 8), np.float32)), _dev(np.ones(8, np.float32))
    hw, h0 = _flat(len(indices))
    yw, Y = _flat(len(rows) * 8)
    with pytest.raises(NotImplementedError, match="vae_bag_fwd: batch 65536"):
        _call("nrhip_vae_bag_fwd", _p(d_ip), _p(d_ix), _p(d_rows), 65536, 8, _p(W), _p(bias), -1, 1.0, None, SEED, 0, _p(h0),
              _p(Y))
    with pytest.raises(NotImplementedError, match="vae_dwq0_wide: batch 65536"):
        _call("nrhip_vae_dwq0_wide", _p(d_ip), _p(d_ix), _p(d_rows), 65536, 8, _p(h0), _p(Y), _p(W))
    assert np.all(_np(hw) == CANARY) and np.all(_np(yw) == CANARY) and np.all(_np(W) == 1.0)
    _call("nrhip_vae_bag_fwd", None, None, None, 0, 8, None, None, -1, 1.0, None, SEED, 0, None, None)
    _call("nrhip_vae_dwq0_wide", None, None, None, 0, 8, None, None, None)
    _call("nrhip_act_bwd", None, None, 0, 0, None)
    _call("nrhip_vae_sample", None, 0, 8, None, 1.0, SEED, 0, None, None, None)
    _call("nrhip_vae_sample_bwd", None, None, None, 0, 8, 0.2, None)
    _call("nrhip_vae_softmax_dlogits", None, 64, 0, 8, None, None, None, None)
    _call("nrhip_transpose2d", None, 8, 0, 8, None, 1)
    _call("nrhip_gemm_f32", None, 8, 0, None, 8, 0, 0, 8, 4, None, 8, 0, None, -1, 1, None, 0)
    # K = 0: A and B are empty tensors (NULL) and are not read; C (+)= 0, then bias and activation
    b5 = np.array([-2.0, -1.0, 0.0, 1.0, 2.0], np.float32)
    for layouts in ((0, 0), (1, 1)):
        cw, c = _wide(8, 5)
        _call("nrhip_gemm_f32", None, 8, layouts[0], None, 5, layouts[1], 8, 5, 0, _p(c), c.stride(0), 0, _p(_dev(b5)), 2, 1,
              None, 0)
        _bits(_np(c), np.tile(np.maximum(b5, 0), (8, 1)), "K = 0: relu(bias)")
        assert _intact(cw, 5)
        _call("nrhip_gemm_f32", None, 8, layouts[0], None, 5, layouts[1], 8, 5, 0, _p(c), c.stride(0), 1, None, -1, 1, None, 0)
        _bits(_np(c), np.tile(np.maximum(b5, 0), (8, 1)), "K = 0, accumulate: C unchanged")
        assert _intact(cw, 5)
    with pytest.raises(ValueError, match="gemm_f32"):                  # a product with a NULL operand is still refused
        _call("nrhip_gemm_f32", None, 8, 0, _p(W), 8, 0, 8, 5, 2, _p(Y), 5, 0, None, -1, 1, None, 0)
    with pytest.raises(ValueError, match="vae_bag_fwd"):               # work with a NULL operand is still refused
        _call("nrhip_vae_bag_fwd", _p(d_ip), _p(d_ix), _p(d_rows), 2, 8, None, _p(bias), -1, 1.0, None, SEED, 0, _p(h0), _p(Y))
    with pytest.raises(ValueError, match="act_bwd"):
        _call("nrhip_act_bwd", None, None, 4, 0, None)
    assert np.all(_np(hw) == CANARY) and np.all(_np(yw) == CANARY)


# ================================================================== C. the GEMM's split tail, 128 tile and transpose
def _gemm(hA, a_kminor, hB, b_kminor, M, N, K, C0, splits, bias=None, act=-1, short_ws=False):
    """operands with 3 columns of padding, C a column block of a [M][N + 4] buffer; the workspace is exactly
    nrhip_gemm_workspace_bytes (canaries behind it) -> C as numpy; or one float short: the call must be refused with
    the workspace status and leave C and the workspace as they were"""
    from neurec_amd._lib import call, NeuRecHipError
    pad = lambda a: np.concatenate([a, np.full((a.shape[0], 3), CANARY, np.float32)], axis=1)
    A = pad(hA if a_kminor else np.ascontiguousarray(hA.T))          # [M][K + 3] or [K][M + 3]
    B = pad(hB if b_kminor else np.ascontiguousarray(hB.T))
    dA, dB = _dev(A), _dev(B)
    cw, c = _wide(M, N, C0, before=1, after=3)
    nbytes = C.c_size_t(0)
    call("nrhip_gemm_workspace_bytes", M, N, splits, C.byref(nbytes))
    chunks = -(-splits // R.RED_CHUNK) if splits > 2 * R.RED_CHUNK else 0
    assert nbytes.value == (4 * (splits + chunks) * M * N if splits > 1 else 0)
    n_ws = nbytes.value // 4 - (1 if short_ws else 0)
    wsw, ws = _flat(max(n_ws, 1))
    go = lambda: _call("nrhip_gemm_f32", _p(dA), A.shape[1], a_kminor, _p(dB), B.shape[1], b_kminor, M, N, K, _p(c),
                       c.stride(0), int(C0 is not None), None if bias is None else _p(_dev(bias)), act, splits,
                       _p(ws) if splits > 1 else None, 4 * n_ws)
    if short_ws:
        before = _np(cw)
        with pytest.raises(NeuRecHipError, match="status 4"):
            go()
        _bits(_np(cw), before, "C after a refused call")
        assert np.all(_np(wsw) == CANARY)
        return None
    go()
    assert _intact(cw, N, 1) and _tail_intact(wsw, max(n_ws, 1))
    return _np(c)


SPLIT_CASES = [(24, 40, 1040, 65), (64, 64, 1040, 65), (24, 40, 1000, 100), (64, 64, 1000, 100), (24, 40, 20000, 100),
               (64, 64, 20000, 100), (64, 64, 70839, 277)]


@pytest.mark.parametrize("M,N,K,splits", SPLIT_CASES)
def test_gemm_two_level_split_reduction_bit_exact(M, N, K, splits):
    """splits > 64: the parts are summed in chunks of 32 (gemm_split_chunks_kernel), the chunk sums in order — 65 parts
    (a last chunk of one), used = 63 <= 64 < splits = 100 (two chunks, the second partial), 97 parts, and the
    production dW shape 64 x 64 over 70,839 rows in 277 parts — with accumulate 0 and 1 (C first, then the chunk sums):
    bit-equal to the restated association; the workspace of exactly nrhip_gemm_workspace_bytes ((splits + chunks)
    slabs) is enough, nothing is written behind it, and one a float short is refused with nothing written"""
    rs = np.random.RandomState(M + K + splits)
    A, B = rs.randn(M, K).astype(np.float32), rs.randn(N, K).astype(np.float32)
    C0 = rs.randn(M, N).astype(np.float32) * 50
    assert splits > 2 * R.RED_CHUNK
    for acc in (None, C0):
        got = _twice(lambda: (_gemm(A, 0, B, 0, M, N, K, acc, splits),))[0]        # both k-major: the dW call
        _bits(got, R.gemm(A, B, splits, acc), ("split", M, N, K, splits, acc is not None))
    for acc in (None, C0):
        _gemm(A, 0, B, 0, M, N, K, acc, splits, short_ws=True)


def test_gemm_two_level_split_with_bias_and_tanh():
    """the epilogue behind the two-level reduction: (C +) chunk sums, + bias, tanh — relu bit for bit, tanhf by the rule"""
    M, N, K, splits = 24, 40, 20000, 100
    rs = np.random.RandomState(8)
    A, B = (0.01 * rs.randn(M, K)).astype(np.float32), rs.randn(N, K).astype(np.float32)
    bias, C0 = rs.randn(N).astype(np.float32), rs.randn(M, N).astype(np.float32)
    f = lambda a: a.astype(np.float64)
    _bits(_twice(lambda: (_gemm(A, 1, B, 0, M, N, K, C0, splits, bias, 2),))[0], R.gemm(A, B, splits, C0, bias, 2),
          "bias + relu")
    got = _twice(lambda: (_gemm(A, 1, B, 0, M, N, K, C0, splits, bias, 0),))[0]
    _within("gemm", "two-level split + bias + tanh", got, R.gemm(A, B, splits, C0, bias, 0),
            R.gemm(f(A), f(B), splits, f(C0), f(bias), 0))


@functools.lru_cache(maxsize=None)
def _tile128_case(M, N, K, splits, layout):
    """other operands in every layout: a tile row a launch forgets to write must not find the right values left in LDS
    by the launch of the layout before"""
    rs = np.random.RandomState(M + N + K + layout)
    A, B = rs.randn(M, K).astype(np.float32), rs.randn(N, K).astype(np.float32)
    C0 = rs.randn(M, N).astype(np.float32)
    out = {"A": A, "B": B, "C0": C0, "plain": R.gemm(A, B, splits), "acc": R.gemm(A, B, splits, C0)}
    if splits == 1:
        from oracle import native
        assert np.array_equal(out["plain"], native.score_gemm(A, None, B))
    return R._frozen(out)


@pytest.mark.parametrize("a_kminor,b_kminor", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("M,N,K,splits", [(129, 16384, 17, 1), (129, 129, 1024, 64)])
def test_gemm_128_tile_in_every_layout_bit_exact(M, N, K, splits, a_kminor, b_kminor):
    """shapes that take the 128 x 128 tile (2 x 128 x 1 and 2 x 2 x 64 >= 256 tiles; PER = 8 slots per thread, RS = 2)
    with a last tile of one row and one column, a partial k tile (K = 17) and 64 splits of one k tile each, in the four
    operand layouts with accumulate 0 and 1, padded lda / ldb / ldc with canaries: splits = 1 is oracle.native.
    score_gemm bit for bit, continued from C when accumulating; the split cases equal the restated association.  Every
    layout has operands of its own (with shared ones a k row that a wrong RS never stores was found in LDS, left there
    by the preceding layout's launch, and the K = 17 case passed)"""
    assert M > 64 and N > 64 and -(-M // 128) * -(-N // 128) * splits >= 256
    c = _tile128_case(M, N, K, splits, 2 * a_kminor + b_kminor)
    for key, C0 in (("plain", None), ("acc", c["C0"])):
        got = _twice(lambda: (_gemm(c["A"], a_kminor, c["B"], b_kminor, M, N, K, C0, splits),))[0]
        _bits(got, c[key], ("128 tile", M, N, K, splits, a_kminor, b_kminor, key))


@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 65), (64, 64), (65, 63), (130, 200)])
def test_transpose2d_leaves_the_padding_alone(rows, cols):
    """ld_src > cols, ld_dst > rows, the destination pre-filled with the canary: dst[c][r] = src[r][c] and every
    padding element of the destination is still the canary"""
    rs = np.random.RandomState(rows + cols)
    X = rs.randn(rows, cols).astype(np.float32)

    def run():
        sw, src = _wide(rows, cols, X)
        dw, dst = _wide(cols, rows, before=1, after=2)
        _call("nrhip_transpose2d", _p(src), src.stride(0), rows, cols, _p(dst), dst.stride(0))
        assert _intact(sw, cols)
        return (_np(dw),)
    want = np.full((cols, rows + 3), CANARY, np.float32)
    want[:, 1:1 + rows] = X.T
    _bits(_twice(run)[0], want, ("transpose2d", rows, cols))
