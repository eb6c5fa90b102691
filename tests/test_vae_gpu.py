"""The narrow Mult-VAE kernels called directly (csrc/vae.hip, csrc/vae_fused.hip and nrhip_vae_step of
csrc/eval_pipeline.hip, through the engine wrappers) against tests/vae_restatement.py: bit equality with the float32
restatement wherever the order of operations is documented and no device libm function is involved, the float64
restatement within 4 x (float32 restatement's own distance) + 1e-5 max|want| elsewhere (expf, tanhf, logf, cosf outputs,
the reassociated decoder sums and the float atomics of vae_dwq0), canary rows beyond the batch in every output, a canary
in every CSR position of h0val, and every case run twice for the same bits (vae_dwq0 excepted: float atomics)."""
import ctypes as C
import functools

import numpy as np
import pytest

import vae_restatement as V

pytestmark = pytest.mark.gpu

CANARY = 7.0
PAD_ROWS = 2
WORST = {}              # section -> (largest device err / reference f32 err seen, where)
F4, F8 = np.float32, np.float64

_LIVE = []              # device copies made by _dev, held until the test ends


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


def _within(section, what, got, w32, w64):
    """device err <= 4 x reference f32 err + 1e-5 max|want|, printed as test_dense_gpu.py prints it"""
    got, w32, w64 = (np.asarray(x, np.float64) for x in (got, w32, w64))
    assert got.shape == w64.shape == w32.shape, (what, got.shape, w32.shape, w64.shape)
    if not got.size:
        return
    assert np.all(np.isfinite(got)), what
    err, bar = np.abs(got - w64).max(), np.abs(w32 - w64).max()
    if bar > 0 and err / bar > WORST.get(section, (0.0, ""))[0]:
        WORST[section] = (err / bar, what)
    print("%s: device err %.3g, reference f32 err %.3g, 1e-5 max|want| %.3g (largest ratio of %s so far %.3g at %s)"
          % ((what, err, bar, 1e-5 * np.abs(w64).max(), section) + WORST.get(section, (0.0, ""))))
    assert err <= 4 * bar + 1e-5 * np.abs(w64).max(), (what, err, bar)


def _rows_buf(B, w):
    """[B + 2][w] (w None: [B + 2]) of canaries: (whole, the first B rows)"""
    import torch
    whole = torch.full((B + PAD_ROWS,) + (() if w is None else (w,)), CANARY, device="cuda")
    _LIVE.append(whole)
    return whole, whole[:B]


def _flat(n, extra=8, fill=CANARY):
    import torch
    whole = torch.full((n + extra,), fill, device="cuda")
    _LIVE.append(whole)
    return whole, whole[:n]


def _pad_intact(whole, n):
    return bool(np.all(_np(whole)[n:] == CANARY))


def _twice(run):
    a, b = run(), run()
    assert len(a) == len(b)
    for k in (a if isinstance(a, dict) else range(len(a))):
        _bits(a[k], b[k], ("repeat", k))
    return a


@functools.lru_cache(maxsize=None)
def _csr():
    from neurec_amd import engine as E
    indptr, indices = V.bag_csr()
    return E.DeviceCSR(np.array(indptr), np.array(indices), V.BAG_ITEMS)        # copies: the frozen arrays are read-only


ENC_OUT = ("H1", "MU", "LOGVAR", "EPSSTD", "ZS", "G1", "KLb")


# ================================================================== the encoder
def _encode(rows, P, h, z, act, keep, is_training, drop, eps, with_h0, step=3):
    """-> dict of the seven outputs (their B rows) and `h0` (the whole CSR's h0val, canaries where nothing was
    written; None without it); canary rows checked"""
    from neurec_amd import engine as E
    B, nnz = len(rows), _csr().nnz
    widths = {"H1": h, "MU": z, "LOGVAR": z, "EPSSTD": z, "ZS": z, "G1": h, "KLb": None}
    bufs = {k: _rows_buf(B, w) for k, w in widths.items()}
    h0w, h0 = _flat(nnz) if with_h0 else (None, None)
    E.vae_encode(_csr(), _dev(rows), P["Wq0"], P["bq0"], P["Wq1"], P["bq1"], P["Wp0"], P["bp0"], act, keep, is_training,
                 V.SEED, step, [bufs[k][1] for k in ENC_OUT], drop_given=drop, eps_given=eps, h0val=h0)
    for k in ENC_OUT:
        assert _pad_intact(bufs[k][0], B), k
    out = {k: _np(bufs[k][1]) for k in ENC_OUT}
    if with_h0:
        assert _pad_intact(h0w, nnz)
        out["h0"] = _np(h0)
    return out


def _h0_check(got_h0, want_at_pos, pos, what):
    _bits(got_h0[pos], want_at_pos, what + ("h0val",))
    rest = np.ones(len(got_h0), bool)
    rest[pos] = False
    assert np.all(got_h0[rest] == CANARY), what + ("h0val outside the batch",)


@pytest.mark.parametrize("h,z", V.WIDTHS)
def test_encode_against_the_restatement(h, z):
    """every batch (the long rows: 2, 5 and 64 segments, seg_len 257 and 258; a user twice; one row; 3 .. 130 rows) x
    four activations with the mask and the noise given: h0val on the batch's positions bit-equal, everything before the
    first libm call bit-equal under relu / identity (H1, MU, LOGVAR; ZS and G1 too at is_training = 0), the rest within
    the bound; h0val elsewhere and the canary rows untouched; h0val = NULL gives the same bits"""
    P = {k: _dev(v) for k, v in V.params(h, z).items()}
    kept, eps = V.given_draws(z)
    kept_d = _dev(kept)
    for name, rows in V.batches().items():
        B = len(rows)
        eps_d = _dev(eps[:B])
        for act in V.ACTS:
            if name not in ("all", "repeat", "b65") and act in ("sigmoid", "identity"):
                continue                                                 # the row counts: two activations are enough
            exact = act in ("relu", "identity")
            for is_training in ((1.0, 0.0) if exact else (1.0,)):
                what = ("encode", h, z, name, act, is_training)
                w32 = V.encode_case(h, z, name, act, 0.8, is_training, F4)
                w64 = V.encode_case(h, z, name, act, 0.8, is_training, F8)
                got = _twice(lambda: _encode(rows, P, h, z, act, 0.8, is_training, kept_d, eps_d, True))
                _h0_check(got["h0"], w32["h0val"], w32["pos"], what)
                for k in ENC_OUT:
                    if exact and (k in ("H1", "MU", "LOGVAR") or (is_training == 0.0 and k in ("ZS", "G1"))):
                        _bits(got[k], w32[k], what + (k,))
                    else:
                        _within("encode", "%s %s" % (what, k), got[k], w32[k], w64[k])
                if name in ("all", "repeat") and is_training == 1.0:     # the evaluation path: no h0val
                    bare = _encode(rows, P, h, z, act, 0.8, is_training, kept_d, eps_d, False)
                    for k in ENC_OUT:
                        _bits(bare[k], got[k], what + (k, "h0val NULL"))


@pytest.mark.parametrize("h,z", [(32, 16), (20, 5), (1, 1)])
def test_encode_device_draws(h, z):
    """keep 0.8 without given draws: h0val is the restated mask's value bit for bit (two steps differ), and the noise
    read back as EPSSTD / exp(LOGVAR / 2) is the restated Box-Muller draw within the bound; keep 1 draws nothing"""
    P = {k: _dev(v) for k, v in V.params(h, z).items()}
    indptr, _ = V.bag_csr()
    nnz = int(indptr[-1])
    for name in ("all", "repeat"):
        rows = V.batches()[name]
        B = len(rows)
        pos = V.encode_case(h, z, name, "identity", 1.0, 1.0, F4)["pos"]
        masks = {}
        for step in (3, 4):
            got = _twice(lambda: _encode(rows, P, h, z, "identity", 0.8, 1.0, None, None, True, step=step))
            masks[step] = V.keep_mask(V.SEED, step, nnz, 0.8)
            _h0_check(got["h0"], V.h0_values(indptr, masks[step], 0.8, F4)[pos], pos, ("drawn", h, z, name, step))
            noise = got["EPSSTD"].astype(F8) / np.exp(0.5 * got["LOGVAR"].astype(F8))
            _within("encode", "drawn noise %s" % ((h, z, name, step),), noise, V.noise(V.SEED, step, B, z, F4),
                    V.noise(V.SEED, step, B, z, F8))
        assert not np.array_equal(masks[3][pos], masks[4][pos]) or len(pos) < 30
        got = _encode(rows, P, h, z, "identity", 1.0, 1.0, None, None, True)
        _h0_check(got["h0"], V.h0_values(indptr, np.ones(nnz, F4), 1.0, F4)[pos], pos, ("keep 1", h, z, name))
        w32 = V.encode_case(h, z, name, "identity", 1.0, 0.0, F4)
        zero = _encode(rows, P, h, z, "identity", 1.0, 0.0, None, None, True)
        for k in ("H1", "MU", "LOGVAR", "ZS", "G1"):
            _bits(zero[k], w32[k], ("keep 1", h, z, name, k))


# ================================================================== add_row_bias
def test_add_row_bias_grid_stride_and_empty():
    """a [33][40,000] column block of a wider canary buffer: 1.32 M elements against the launch's 4,096 x 256 threads,
    so the grid-stride loop takes a second round; bit-equal, padding intact; batch = 0 writes nothing"""
    import torch
    rs = np.random.RandomState(5)
    B, cols, before, after = 33, 40000, 2, 3
    assert B * cols > 4096 * 256
    S, bias = rs.randn(B, cols).astype(F4), rs.randn(cols).astype(F4)
    bias_d = _dev(bias)

    def run():
        wide = torch.full((B + 1, before + cols + after), CANARY, device="cuda")
        view = wide[:B, before:before + cols]
        view.copy_(_dev(S))
        _call("nrhip_add_row_bias", _p(view), view.stride(0), B, cols, _p(bias_d))
        w = _np(wide)
        assert np.all(w[B] == CANARY) and np.all(w[:, :before] == CANARY) and np.all(w[:, before + cols:] == CANARY)
        return (w[:B, before:before + cols],)
    _bits(_twice(run)[0], V.add_row_bias(S, bias), "add_row_bias")
    wide = torch.full((4, 16), CANARY, device="cuda")
    _call("nrhip_add_row_bias", _p(wide), 16, 0, 16, _p(bias_d))
    assert np.all(_np(wide) == CANARY)


# ================================================================== the middle of the backward pass
def _mid(c, B, h, z, act, anneal):
    from neurec_amd import engine as E
    rows = {k: _rows_buf(B, w) for k, w in (("DA3", h), ("DH2", 2 * z), ("DA1", h))}
    flat = {k: _flat(n) for k, n in (("dWp0", z * h), ("dbp0", h), ("dWq1", h * 2 * z), ("dbq1", 2 * z), ("dbq0", h))}
    d = {k: _dev(c[k][:B]) for k in ("dG1", "G1", "H1", "MU", "LOGVAR", "EPSSTD", "ZS")}
    E.vae_mid_backward(B, act, anneal, d["dG1"], d["G1"], d["H1"], d["MU"], d["LOGVAR"], d["EPSSTD"], d["ZS"],
                       _dev(c["Wp0"]), _dev(c["Wq1"]), rows["DA3"][1], rows["DH2"][1], rows["DA1"][1],
                       flat["dWp0"][1].view(z, h), flat["dbp0"][1], flat["dWq1"][1].view(h, 2 * z), flat["dbq1"][1],
                       flat["dbq0"][1])
    for k, (whole, _) in rows.items():
        assert _pad_intact(whole, B), k
    for k, (whole, part) in flat.items():
        assert _pad_intact(whole, part.numel()), k
    out = {k: _np(v[1]) for k, v in rows.items()}
    out.update({k: _np(v[1]) for k, v in flat.items()})
    out["dWp0"], out["dWq1"] = out["dWp0"].reshape(z, h), out["dWq1"].reshape(h, 2 * z)
    return out


@pytest.mark.parametrize("h,z", V.WIDTHS)
def test_mid_backward_against_the_restatement(h, z):
    """four activations x B in 1, 3, 4, 5, 63, 64, 65, 130 (four rows share a workgroup; lanes stride the batch by 64)
    x anneal 0 and 0.2: DA3 and the mu half of DH2 bit-equal, all of DH2 and DA1 bit-equal at anneal 0 and within the
    bound at 0.2 (expf), the five weight gradients bit-equal to the restatement fed with the device's own DA3 / DH2 /
    DA1 — the lane-strided fmaf chain and the wave sum on their own"""
    for act in V.ACTS:
        for B in V.MID_BATCHES:
            c = V.mid_inputs(B, h, z, act)
            args = [c[k] for k in ("dG1", "G1", "H1", "MU", "LOGVAR", "EPSSTD", "Wp0", "Wq1")]
            for anneal in (0.0, 0.2):
                what = ("mid", h, z, act, B, anneal)
                w32 = V.mid_backward(*args, V.ACTS[act], anneal)
                w64 = V.mid_backward(*[a.astype(F8) for a in args], V.ACTS[act], anneal)
                got = _twice(lambda: _mid(c, B, h, z, act, anneal))
                _bits(got["DA3"], w32[0], what + ("DA3",))
                _bits(got["DH2"][:, :z], w32[1][:, :z], what + ("dmu",))
                if anneal == 0.0:
                    _bits(got["DH2"], w32[1], what + ("DH2",))
                    _bits(got["DA1"], w32[2], what + ("DA1",))
                else:
                    _within("mid", "%s DH2" % (what,), got["DH2"], w32[1], w64[1])
                    _within("mid", "%s DA1" % (what,), got["DA1"], w32[2], w64[2])
                names = ("dWp0", "dbp0", "dWq1", "dbq1", "dbq0")
                for k, want in zip(names, V.mid_wgrads(c["ZS"], c["H1"], got["DA3"], got["DH2"], got["DA1"])):
                    _bits(got[k], want, what + (k,))


# ================================================================== dW_q0
@pytest.mark.parametrize("h", [32, 20, 1])
def test_dwq0_against_the_restatement(h):
    """the long rows (a second chunk round above 1,024 items) and the user listed twice: within the bound (float atomics
    in any order); rows of items that no batch row holds stay exactly zero"""
    from neurec_amd import engine as E
    indptr, indices = V.bag_csr()
    hv = V.h0_values(indptr, V.given_draws(16)[0], 0.8, F4)
    hv_d = _dev(hv)
    for name in ("all", "repeat"):
        rows = V.batches()[name]
        DA1 = np.random.RandomState(h).randn(len(rows), h).astype(F4)
        whole, dW = _flat(V.BAG_ITEMS * h)
        dW.zero_()
        E.vae_dwq0(_csr(), _dev(rows), hv_d, _dev(DA1), dW.view(V.BAG_ITEMS, h))
        assert _pad_intact(whole, V.BAG_ITEMS * h)
        got = _np(dW).reshape(V.BAG_ITEMS, h)
        _within("dwq0", "dwq0 %s h=%d" % (name, h), got, V.dwq0(indptr, indices, rows, hv, DA1, V.BAG_ITEMS),
                V.dwq0(indptr, indices, rows, hv.astype(F8), DA1.astype(F8), V.BAG_ITEMS))
        held = np.zeros(V.BAG_ITEMS, bool)
        for u in rows:
            held[indices[indptr[u]:indptr[u + 1]]] = True
        assert name == "all" or not held.all()
        assert not np.any(got[~held])
    whole, dW = _flat(64)
    _call("nrhip_vae_dwq0", _p(_csr().indptr), _p(_csr().indices), _p(_dev(V.batches()["all"])), 0, h, _p(hv_d),
          _p(_dev(np.ones((1, h), F4))), _p(dW))                         # batch = 0
    assert np.all(_np(whole) == CANARY)


# ================================================================== the two decoders
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


DEC_SHAPES = ((1, 1, 1), (33, 31, 32), (257, 100, 20), (513, 70, 32), "tail")


def _dec_outputs(B, I, h):
    return {"nll": _rows_buf(B, None), "dWp1": _flat(I * h), "dbp1": _flat(I), "dg1": _rows_buf(B, h)}


def _dec_read(o, B, I, h):
    assert _pad_intact(o["nll"][0], B) and _pad_intact(o["dg1"][0], B)
    assert _pad_intact(o["dWp1"][0], I * h) and _pad_intact(o["dbp1"][0], I)
    return {"nll": _np(o["nll"][1]), "dWp1": _np(o["dWp1"][1]).reshape(I, h), "dbp1": _np(o["dbp1"][1]),
            "dg1": _np(o["dg1"][1])}


def _slab(c, csr, B, I, h, S_host, junk):
    """the slab form on S = g1 W^T [B][ld] (ld = I padded to 64, as ScoreGemm.new_score_buffer lays it out); the pad
    columns hold `junk`"""
    import torch
    from neurec_amd import engine as E
    ld = (I + 63) // 64 * 64
    S = torch.full((B, ld), junk, device="cuda")
    _LIVE.append(S)
    S[:, :I] = _dev(S_host)
    o = _dec_outputs(B, I, h)
    E.vae_decoder_loss_grad(S, I, _dev(c["b"]), csr, _dev(c["rows"]), _dev(c["G1"]), _dev(c["W"]), o["nll"][1],
                            o["dWp1"][1].view(I, h), o["dbp1"][1], o["dg1"][1], E.vae_workspace(B, I, "cuda"))
    assert np.all(_np(S[:, I:]) == F4(junk))
    _bits(_np(S[:, :I]), S_host, "the slab is only read")
    return _dec_read(o, B, I, h)


def _fused(c, csr, B, I, h, dbg=None):
    from neurec_amd import engine as E
    o = _dec_outputs(B, I, h)
    E.vae_decoder_fused(I, _dev(c["b"]), csr, _dev(c["rows"]), _dev(c["G1"]), _dev(c["W"]), o["nll"][1],
                        o["dWp1"][1].view(I, h), o["dbp1"][1], o["dg1"][1], E.vae_fused_workspace(B, I, "cuda"),
                        dbg_logits=dbg)
    return _dec_read(o, B, I, h)


@pytest.mark.parametrize("kind", V.DEC_KINDS)
@pytest.mark.parametrize("shape", DEC_SHAPES, ids=str)
def test_decoders_against_float64(shape, kind):
    """slab and fused form, each against the float64 statement, on logits of today's scale (unit), spanning more than
    104 per row (wide: the clamp of exp_nonpos engages), all equal (flat: lse = b + log I read back through nll / n_b on
    rows whose n_b is a power of two) and with every positive 30 under the row maximum (buried); the batch holds a user
    without history, a user of every item and one user twice.  `tail`: B = 40, I = 32 (CUs + 3) + 5 — more item tiles
    than the fused kernel has workgroups, the left-over tiles cut by rows.  nll, dW_p1, db_p1 and dg1 within the bound;
    1e30 in the slab's pad columns changes nothing; on unit logits the fused form's logits equal the slab's bit for bit."""
    import torch
    from neurec_amd import engine as E
    B, I, h = (40, 32 * (_cus() + 3) + 5, 32) if shape == "tail" else shape
    if kind == "buried" and I < 31:
        return                                                           # no room for items above every positive
    c = V.decoder_case(B, I, h, kind)
    w32, w64 = V.decoder_want(B, I, h, kind, F4), V.decoder_want(B, I, h, kind, F8)
    csr = E.DeviceCSR(np.array(c["indptr"]), np.array(c["indices"]), I)
    S_host = V.fma_chain(c["G1"], c["W"])
    slab = _twice(lambda: _slab(c, csr, B, I, h, S_host, 0.0))
    junk = _slab(c, csr, B, I, h, S_host, 1e30)
    for k in slab:
        _bits(junk[k], slab[k], ("junk in the pad columns", k))
    fused = _twice(lambda: _fused(c, csr, B, I, h))
    if kind == "unit":
        dbg = torch.full((B, I), float("nan"), device="cuda")
        _bits(_fused(c, csr, B, I, h, dbg=dbg)["nll"], fused["nll"], "dbg_logits changes nothing")
        _bits(_np(dbg), w32["logits"], "fused logits = the k-ascending chain + bias")
        if I >= 31:                                                      # the score GEMM itself: the slab's producer
            Wd = _dev(c["W"])
            gemm = E.ScoreGemm(Wd, B)
            Sg = gemm(_dev(c["G1"]), None, out=gemm.new_score_buffer(B))
            assert torch.equal(dbg, Sg[:, :I] + _dev(c["b"])[None, :])
    for form, got in (("slab", slab), ("fused", fused)):
        for k in ("nll", "dWp1", "dbp1", "dg1"):
            what = "%s %s %s %s" % (form, (B, I, h), kind, k)
            if I == 1:
                # one item: softmax = 1, every output is exactly 0 in both restatements (no yardstick).  The device's
                # softmax is 2^(x log2e - lse log2e) with lse = x: off from 1 by the rounding of one product,
                # 2^-24 |x log2e| ln 2 + 2^-24 — under 2^-22 max(1, |x|), times the operand it is multiplied with
                x = float(np.abs(w64["logits"]).max())
                lim = 2.0 ** -22 * max(1.0, x) * max(1.0, float(np.abs(c["G1"]).max()), float(np.abs(c["W"]).max()))
                print("%s: |device| %.3g (exact value 0, limit %.3g)" % (what, np.abs(got[k]).max(), lim))
                assert np.abs(got[k]).max() <= lim, what
            else:
                _within(form, what, got[k], w32[k], w64[k])
        n = np.diff(c["indptr"])[c["rows"]]
        if kind in ("flat", "wide"):
            live = n > 0
            lse_err = np.abs(got["nll"][live].astype(F8) / n[live] - w64["nll"][live] / n[live])
            print("%s %s %s: lse error read back through nll / n_b: largest %.3g (lse up to %.3g, its float32 ulp %.3g)"
                  % (form, (B, I, h), kind, lse_err.max(), np.abs(w64["lse"]).max(),
                     np.spacing(F4(np.abs(w64["lse"]).max()))))
        if kind == "flat":
            # every logit is 0.25 exactly (W = 0, fmaf(1, b, 0) = b: no bias rounding), lse = 0.25 + log I.  On a row
            # whose n_b is a power of two the read-back nll / n_b = lse - 0.25 adds one rounding of that difference
            # (the n_b equal terms and n_b lse are exact): 1 ulp of lse for the kernel + half an ulp of log I
            pow2 = np.isin(n, V.DEC_POW2)
            assert pow2.any()
            lse = 0.25 + np.log(I)
            tol = np.spacing(F4(lse)) + 0.5 * np.spacing(F4(np.log(I))) if I > 1 else 0.0
            err = np.abs(got["nll"][pow2].astype(F8) / n[pow2] + 0.25 - lse).max()
            print("%s %s flat: |lse - (b + log I)| = %.3g (1 ulp + read-back %.3g)" % (form, (B, I, h), err, tol))
            assert err <= tol, (form, err, tol)


def test_decoders_mid_backward_and_step_accept_an_empty_batch():
    """batch = 0: both decoders, mid_backward and nrhip_vae_step return without a launch and touch nothing"""
    from neurec_amd import engine as E
    B, I, h = 33, 31, 32
    c = V.decoder_case(B, I, h, "unit")
    csr = E.DeviceCSR(np.array(c["indptr"]), np.array(c["indices"]), I)
    rows0, G0 = _dev(c["rows"])[:0], _dev(c["G1"])[:0]
    assert rows0.numel() == 0 and G0.shape == (0, h)
    o = _dec_outputs(0, I, h)
    for k in ("dWp1", "dbp1"):
        o[k][1].fill_(CANARY)
    S = _dev(np.zeros((1, 64), F4))
    E.vae_decoder_loss_grad(S[:0], I, _dev(c["b"]), csr, rows0, G0, _dev(c["W"]), o["nll"][1], o["dWp1"][1].view(I, h),
                            o["dbp1"][1], o["dg1"][1], E.vae_workspace(0, I, "cuda"))
    E.vae_decoder_fused(I, _dev(c["b"]), csr, rows0, G0, _dev(c["W"]), o["nll"][1], o["dWp1"][1].view(I, h),
                        o["dbp1"][1], o["dg1"][1], E.vae_fused_workspace(0, I, "cuda"))
    for k in o:
        assert np.all(_np(o[k][0]) == CANARY), k
    m = V.mid_inputs(3, 20, 5, "tanh")
    got = _mid({k: (v[:0] if k not in ("Wp0", "Wq1") else v) for k, v in m.items()}, 0, 20, 5, "tanh", 0.2)
    for k, v in got.items():
        assert v.size == 0 or np.all(v == CANARY), k
    st = _Step(20, 5, "tanh", 4)
    st.fill_gradients(CANARY)
    st.native(V.batches()["repeat"][:0], 0.2, 0.8, None, None)
    for k, g in st.G.items():
        assert np.all(_np(g) == CANARY), k
    assert np.all(_np(st.buf["stats"]) == CANARY)


# ================================================================== the whole step as one native call
NAMES = ("Wq0", "bq0", "Wq1", "bq1", "Wp0", "bp0", "Wp1t", "bp1")


class _Step:
    """the buffers of one narrow Mult-VAE step on the frozen CSR, and the step issued natively or call by call"""

    def __init__(self, h, z, act, max_batch):
        import torch
        from neurec_amd import engine as E
        self.h, self.z, self.act, self.I = h, z, act, V.BAG_ITEMS
        self.P = {k: _dev(v) for k, v in V.params(h, z).items()}
        new = lambda: {k: torch.zeros_like(v) for k, v in self.P.items()}
        self.G, self.M, self.Vv = new(), new(), new()
        f = lambda *s: torch.full(s, CANARY, device="cuda")
        B = max(max_batch, 1)
        self.buf = {"H1": f(B, h), "MU": f(B, z), "LOGVAR": f(B, z), "EPSSTD": f(B, z), "ZS": f(B, z), "G1": f(B, h),
                    "KLb": f(B), "h0val": f(_csr().nnz), "nll": f(B), "dG1": f(B, h), "DA3": f(B, h), "DH2": f(B, 2 * z),
                    "DA1": f(B, h), "stats": f(2), "regsum": torch.zeros(1, dtype=torch.float64, device="cuda"),
                    "ws": E.vae_fused_workspace(B, self.I, "cuda")}
        _LIVE.extend([self.P, self.G, self.M, self.Vv, self.buf])

    def fill_gradients(self, value):
        for g in self.G.values():
            g.fill_(value)

    def native(self, rows, anneal, keep, drop, eps, step=3):
        from neurec_amd._lib import VaeStepArgs
        a = VaeStepArgs()
        csr = _csr()
        a.indptr, a.indices = csr.indptr.data_ptr(), csr.indices.data_ptr()
        a.n_items, a.h, a.z, a.act = self.I, self.h, self.z, V.ACTS[self.act]
        for k, n in enumerate(NAMES):
            a.P[k], a.G[k], a.M[k], a.V[k] = (d[n].data_ptr() for d in (self.P, self.G, self.M, self.Vv))
            a.sizes[k] = self.P[n].numel()
        for k, t in self.buf.items():
            setattr(a, k, t.data_ptr())
        a.ws_bytes = self.buf["ws"].numel()
        a.drop_given = drop.data_ptr() if drop is not None else None
        a.eps_given = eps.data_ptr() if eps is not None else None
        a.reg, a.beta1, a.beta2, a.adam_eps, a.seed = 0.0, 0.9, 0.999, 1e-8, V.SEED
        rows_d = _dev(rows) if len(rows) else None
        _call("nrhip_vae_step", C.byref(a), _p(rows_d), len(rows), float(anneal), float(keep), 1e-3, C.c_uint64(step),
              1, 0)

    def one_by_one(self, rows, anneal, keep, drop, eps, step=3):
        from neurec_amd import engine as E
        B, P, G, b = len(rows), self.P, self.G, self.buf
        rows_d = _dev(rows)
        E.vae_encode(_csr(), rows_d, P["Wq0"], P["bq0"], P["Wq1"], P["bq1"], P["Wp0"], P["bp0"], self.act, keep, 1.0,
                     V.SEED, step, [b[k][:B] for k in ENC_OUT], drop_given=drop, eps_given=eps, h0val=b["h0val"])
        E.vae_decoder_fused(self.I, P["bp1"], _csr(), rows_d, b["G1"][:B], P["Wp1t"], b["nll"][:B], G["Wp1t"], G["bp1"],
                            b["dG1"][:B], b["ws"])
        E.vae_mid_backward(B, self.act, anneal, b["dG1"][:B], b["G1"][:B], b["H1"][:B], b["MU"][:B], b["LOGVAR"][:B],
                           b["EPSSTD"][:B], b["ZS"][:B], P["Wp0"], P["Wq1"], b["DA3"][:B], b["DH2"][:B], b["DA1"][:B],
                           G["Wp0"], G["bp0"], G["Wq1"], G["bq1"], G["bq0"])
        E.vae_dwq0(_csr(), rows_d, b["h0val"], b["DA1"][:B], G["Wq0"])


def test_native_step_equals_the_entry_points_one_by_one():
    """nrhip_vae_step (apply = 0) on the batch holding the 1,025-item user and the user listed twice, h = 20, z = 5:
    every gradient bit-equal to the same entry points issued one by one, but G[Wq0] (float atomics in both), which is
    within the bound of the restated scatter of the step's own DA1 and h0val"""
    h, z, anneal, keep = 20, 5, 0.2, 0.8
    rows = V.batches()["repeat"]
    indptr, indices = V.bag_csr()
    kept, eps = V.given_draws(z)
    kept_d, eps_d = _dev(kept), _dev(eps[:len(rows)])
    a, b = _Step(h, z, "tanh", len(rows)), _Step(h, z, "tanh", len(rows))
    a.native(rows, anneal, keep, kept_d, eps_d)
    b.one_by_one(rows, anneal, keep, kept_d, eps_d)
    for k in NAMES[1:]:
        _bits(_np(a.G[k]), _np(b.G[k]), ("step", k))
    for k in ("H1", "MU", "LOGVAR", "EPSSTD", "ZS", "G1", "KLb", "nll", "dG1", "DA3", "DH2", "DA1", "h0val"):
        _bits(_np(a.buf[k]), _np(b.buf[k]), ("step", k))
    assert np.any(_np(a.G["Wp1t"])) and np.any(_np(a.G["bq0"]))
    hv, DA1 = _np(a.buf["h0val"]), _np(a.buf["DA1"])
    pos = V.encode_case(h, z, "repeat", "tanh", 0.8, 1.0, F4)["pos"]
    hv0 = np.zeros_like(hv)
    hv0[pos] = hv[pos]                                                   # (canaries elsewhere: never read)
    w32 = V.dwq0(indptr, indices, rows, hv0, DA1, V.BAG_ITEMS)
    w64 = V.dwq0(indptr, indices, rows, hv0.astype(F8), DA1.astype(F8), V.BAG_ITEMS)
    for name, s in (("native", a), ("one by one", b)):
        _within("dwq0", "step G[Wq0] %s" % name, _np(s.G["Wq0"]), w32, w64)


# ================================================================== refusals (nothing is launched)
def test_refusals_launch_nothing():
    """h = 33, z = 17, keep = 0, act = 4, a short workspace, and a slab or bias the statistics kernel could not read as
    float4 (odd row stride, pointers off 16 bytes) each raise the mapped Python error before any launch"""
    import torch
    from neurec_amd import engine as E
    from neurec_amd._lib import NeuRecHipError
    x = torch.zeros(4096, device="cuda")
    xi = torch.zeros(64, dtype=torch.int32, device="cuda")
    xl = torch.zeros(64, dtype=torch.int64, device="cuda")

    def encode(h, z, act, keep):
        _call("nrhip_vae_encode", _p(xl), _p(xi), _p(xi), 1, h, z, _p(x), _p(x), _p(x), _p(x), _p(x), _p(x), act, keep,
              None, None, 1.0, C.c_uint64(1), C.c_uint64(0), None, _p(x), _p(x), _p(x), _p(x), _p(x), _p(x), _p(x))
    with pytest.raises(NotImplementedError, match="hidden 33"):
        encode(33, 16, 0, 1.0)
    with pytest.raises(NotImplementedError, match="latent 17"):
        encode(32, 17, 0, 1.0)
    with pytest.raises(ValueError, match="vae_encode"):
        encode(32, 16, 0, 0.0)
    with pytest.raises(ValueError, match="vae_encode"):
        encode(32, 16, 4, 1.0)
    with pytest.raises(NotImplementedError, match="vae_mid_backward"):
        _call("nrhip_vae_mid_backward", 1, 33, 16, 0, 0.0, *([_p(x)] * 17))
    with pytest.raises(NotImplementedError, match="vae_mid_backward"):
        _call("nrhip_vae_mid_backward", 1, 32, 17, 0, 0.0, *([_p(x)] * 17))
    with pytest.raises(NotImplementedError, match="hidden 33"):
        _call("nrhip_vae_decoder_fused", 1, 8, 33, _p(x), _p(x), _p(x), _p(xl), _p(xi), _p(xi), _p(x), _p(x), _p(x),
              _p(x), _p(x), 1 << 30, None)
    short = torch.zeros(16, dtype=torch.uint8, device="cuda")
    with pytest.raises(NeuRecHipError, match="workspace too small"):
        _call("nrhip_vae_decoder_fused", 1, 8, 32, _p(x), _p(x), _p(x), _p(xl), _p(xi), _p(xi), _p(x), _p(x), _p(x),
              _p(x), _p(short), short.numel(), None)

    def slab(S, ld, bias, ws=short):
        _call("nrhip_vae_decoder_loss_grad", _p(S), ld, 1, 8, 32, _p(bias), _p(xl), _p(xi), _p(xi), _p(x), _p(x), _p(x),
              _p(x), _p(x), _p(x), _p(ws), ws.numel())
    with pytest.raises(NeuRecHipError, match="workspace too small"):
        slab(x, 64, x)
    assert x.data_ptr() % 16 == 0
    with pytest.raises(ValueError, match="float4"):
        slab(x, 9, x)                                                    # rows 36 bytes apart
    with pytest.raises(ValueError, match="float4"):
        slab(x[1:], 64, x)                                               # the slab 4 bytes off
    with pytest.raises(ValueError, match="float4"):
        slab(x, 64, x[2:])                                               # the bias 8 bytes off
    with pytest.raises(ValueError, match="bad arguments"):
        slab(x, 4, x)                                                    # ld < cols
    assert not x.any()
