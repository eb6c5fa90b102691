"""The restatement of the narrow NGCF layer (tests/ngcf_restatement.py) checked on the host, so that
test_ngcf_layer_gpu.py does not compare the kernels of csrc/dense.hip with a wrong copy of themselves: the float64
functions against torch.autograd in float64 on the layer written with torch operations (1e-12 max|want|) and against
oracle.train on a one-layer problem, the float32 forms within ordinary rounding of the float64 ones, the chains against
the C fmaf of oracle.native.score_gemm, the 16-bit mask draw against the hash in Python integers, and the constructed
inputs shown to hold what they claim."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import native, train
import ngcf_restatement as N
from test_dense_cpu import _rounding

F4, F8 = np.float32, np.float64
AUTOGRAD_TOL = 1e-12          # relative to max|want|: float64 keeps 2^-53 = 1.1e-16 per operation
SEED = 2017


def _close(what, got, want, tol=AUTOGRAD_TOL):
    got, want = np.asarray(got, F8), np.asarray(want, F8)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, top = np.abs(got - want).max(), np.abs(want).max()
    print("%s: largest difference %.3g, max|want| %.3g, bound %.3g" % (what, err, top, tol * top))
    assert err <= tol * top, (what, err, top)


def test_chains_equal_the_c_fmaf_chain():
    """T = x W + b and y = g W^T as this file's chains, against oracle.native.score_gemm (k-ascending fmaf from 0)"""
    c = N.layer_inputs(65, "biased")
    zero = np.zeros(N.D, F4)
    assert np.array_equal(N._affine(c["S"], c["Wg"], zero), native.score_gemm(c["S"], None, np.ascontiguousarray(c["Wg"].T)))
    assert np.array_equal(N._affine_t(c["d_out"], c["Wb"]), native.score_gemm(c["d_out"], None, c["Wb"]))
    assert not np.array_equal(N._affine(c["S"], c["Wg"], c["bg"]), N._affine(c["S"], c["Wg"], zero) + c["bg"])   # from the bias
    assert np.array_equal(N._row_chain(c["S"], c["ego"]), native.score_gemm(c["S"], None, c["ego"]).diagonal())


@pytest.mark.parametrize("kind", N.KINDS)
@pytest.mark.parametrize("keep", N.KEEPS)
@pytest.mark.parametrize("with_next", (False, True))
def test_float64_restatement_equals_autograd(kind, keep, with_next):
    """the loss is a random linear functional of out plus (with_next) one of ego_out, which stands in for d_ego_next.
    The case holds a fully masked row (ss = 0), in "unbiased" a row with 0 < ss < 1e-12 and a row of exactly zero
    pre-activations; no row sits at ss = 1e-12.  Every output is held to 1e-12 max|want|, and the rows other than the
    small one (its gradient is 1e6 times an ordinary one) once more to 1e-12 of their own maximum."""
    n = 65
    c = N.layer_inputs(n, kind)
    ego, S, Wg, bg, Wb, bb, mask = N.layer_args(c, F8)
    G, Gn = c["d_out"].astype(F8), (c["d_ego_next"].astype(F8) if with_next else None)
    k8 = float(F4(keep))
    t = {k: torch.tensor(v, requires_grad=True) for k, v in zip(("ego", "S", "Wg", "bg", "Wb", "bb"), (ego, S, Wg, bg, Wb, bb))}
    lrelu = lambda x: torch.where(x > 0, x, x * float(N.LEAKY))
    T1 = t["S"] @ t["Wg"] + t["bg"]
    T2 = (t["ego"] * t["S"]) @ t["Wb"] + t["bb"]
    T1.retain_grad(), T2.retain_grad()
    z = torch.where(torch.tensor(mask != 0), (lrelu(T1) + lrelu(T2)) / k8, torch.zeros((), dtype=torch.float64))
    ss = (z * z).sum(1, keepdim=True)
    out = z / torch.sqrt(torch.clamp(ss, min=float(N.NORM_EPS)))
    loss = (out * torch.tensor(G)).sum()
    if with_next:
        loss = loss + (z * torch.tensor(Gn)).sum()
    loss.backward()
    ss_np = ss.detach().numpy()[:, 0]
    assert (ss_np == 0).any() and (ss_np > 1e-6).any() and not np.any(np.abs(ss_np - 1e-12) < 1e-13)
    if kind == "unbiased":
        assert 0 < ss_np[N.ROW_TINY] < 1e-12 and not T1.detach().numpy()[N.ROW_ZERO_PRE].any()

    got_e, got_o = N.layer_fwd(ego, S, Wg, bg, Wb, bb, mask, keep)
    _close("ego_out", got_e, z.detach().numpy())
    _close("out", got_o, out.detach().numpy())
    rows = N.layer_bwd_rows(ego, S, Wg, bg, Wb, bb, mask, keep, G, Gn)
    want_rows = [t["S"].grad.numpy(), t["ego"].grad.numpy(), T1.grad.numpy(), T2.grad.numpy()]
    plain = np.arange(n) != N.ROW_TINY
    for name, got, want in zip(("dS", "d_ego_direct", "dT1", "dT2"), rows, want_rows):
        assert got.dtype == F8
        _close(name, got, want)
        _close(name + " without the small row", got[plain], want[plain])
    grads, terms = N.layer_wgrads(ego, S, rows[2], rows[3])
    for name, got, a, want in zip(("dWg", "dbg", "dWb", "dbb"), grads, terms, (t[k].grad.numpy() for k in ("Wg", "bg", "Wb", "bb"))):
        _close(name, got, want)
        assert np.all(a >= np.abs(got)) and a.shape == got.shape


def test_float64_restatement_equals_the_oracle():
    """One NGCF layer of oracle.train on a small graph, S = A E taken from the oracle's cache: forward (E', out), and
    of ngcf_loss_and_grads' layer loop the four weight gradients and dE0 = dOut[:, :16] + d_ego_direct + A^T dS, with
    dOut restated from the oracle's BPR head.  One masked-out row.
    Bound: the oracle writes the slope 0.2 and the floor 1e-12 as float64, the restatement rounds both to float32 as
    the kernels hold them: relative changes of 1.5e-8 and 4e-9.  Every output is a product of at most three factors
    that depend on the slope (z, the normalisation, the gradient's own slope factor) and the floor enters through
    1 / sqrt alone, so 8 x the larger relative change, relative to the largest value, covers it; float64 rounding
    (1e-12) is added.  keep is handed to the oracle as the float32 value, so it contributes nothing."""
    rs = np.random.RandomState(5)
    U, I, B, reg = 40, 30, 24, 0.01
    Rm = sp.random(U, I, 0.15, random_state=5, format="csr", dtype=F4)
    Rm.data[:] = rs.randint(1, 6, Rm.nnz)
    A = train.ngcf_adjacency(Rm, "norm").astype(F8)
    At = A.T.tocsr()
    n = U + I
    c = N.layer_inputs(n, "biased")
    E0, Wg, bg, Wb, bb = (c[k].astype(F8) for k in ("ego", "Wg", "bg", "Wb", "bb"))
    mask = (c["mask"] != 0).astype(np.uint8)
    assert not mask[N.ROW_MASKED].any()
    keep = float(F4(0.9))
    W = [(Wg, bg[None, :], Wb, bb[None, :])]
    bu, bp, bn = (rs.randint(0, m, B) for m in (U, I, I))
    out, cache = train.ngcf_forward(A, E0, W, [mask.astype(F8)], keep)
    _, dE0, wg = train.ngcf_loss_and_grads(A, At, E0, W, [mask.astype(F8)], keep, U, bu, bp, bn, reg)
    S = cache[0][1]
    slope = abs(float(N.LEAKY) - 0.2) / 0.2
    floor = abs(float(N.NORM_EPS) - 1e-12) / 1e-12
    assert 1e-8 < slope < 2.0 ** -24 and 1e-9 < floor < 2.0 ** -24
    tol = 8 * max(slope, floor) + 1e-12
    got_e, got_o = N.layer_fwd(E0, S, Wg, bg, Wb, bb, mask, keep)
    _close("ego_out", got_e, cache[0][5], tol)
    _close("out", got_o, out[:, N.D:], tol)
    # the BPR head of ngcf_loss_and_grads, on the oracle's own output
    iu, ii, ij = bu, U + bp, U + bn
    eu, ei, ej = out[iu], out[ii], out[ij]
    _, g = train.bpr_terms(np.sum(eu * ei, axis=1) - np.sum(eu * ej, axis=1))
    dOut = np.zeros_like(out)
    np.add.at(dOut, iu, g[:, None] * (ei - ej) + reg * eu)
    np.add.at(dOut, ii, g[:, None] * eu + reg * ei)
    np.add.at(dOut, ij, -g[:, None] * eu + reg * ej)
    dS, dEd, dT1, dT2 = N.layer_bwd_rows(E0, S, Wg, bg, Wb, bb, mask, keep, dOut[:, N.D:], None)
    grads, _ = N.layer_wgrads(E0, S, dT1, dT2)
    for name, got, want in zip(("dWg", "dbg", "dWb", "dbb"), grads, wg[0]):
        _close(name, got, np.asarray(want).reshape(got.shape), tol)
    _close("dE0", dOut[:, :N.D] + dEd + At @ dS, dE0, tol)
    assert np.abs(dE0).max() > 1e-3 and np.abs(grads[0]).max() > 1e-3


@pytest.mark.parametrize("kind", N.KINDS)
def test_float32_restatement_lies_within_rounding_of_float64(kind):
    """ops: a generous count of the roundings an output passes through — the 17 of a pre-activation chain, 3 to z,
    16 + 3 through the norm (40 forward); the dot's 16, 6 to dT, a transposed chain's 16 and 2 more on top (80
    backward).  The rows other than the small one are compared among themselves: its gradient is 1e6 times theirs."""
    n, keep = 257, 0.9
    c = N.layer_inputs(n, kind)
    a4, a8 = N.layer_args(c), N.layer_args(c, F8)
    e4, o4 = N.layer_fwd(*a4, keep)
    e8, o8 = N.layer_fwd(*a8, keep)
    assert e4.dtype == o4.dtype == F4 and e8.dtype == o8.dtype == F8
    _rounding("ego_out", e4, e8, 20)
    _rounding("out", o4, o8, 40)
    plain = np.arange(n) != N.ROW_TINY
    for nxt in (None, "d_ego_next"):
        b4 = N.layer_bwd_rows(*a4, keep, c["d_out"], None if nxt is None else c[nxt])
        b8 = N.layer_bwd_rows(*a8, keep, c["d_out"].astype(F8), None if nxt is None else c[nxt].astype(F8))
        for name, x4, x8 in zip(("dS", "d_ego_direct", "dT1", "dT2"), b4, b8):
            _rounding(name, x4, x8, 120)
            _rounding(name + " without the small row", x4[plain], x8[plain], 120)


def test_draw_mask16_equals_the_integer_hash():
    """every byte of 70 rows against the Python-integer form; at 4,097 x 16 draws the mean lies within 0.01 of keep
    (its standard deviation is sqrt(0.09 / 65552) = 0.0012); keep = 1.0 keeps everything (the largest draw is
    65535 / 65536); another step or layer gives another mask"""
    for keep in (0.9, 0.5, 1.0):
        m = N.draw_mask16(SEED, 3, 1, 70, keep)
        assert m.dtype == np.uint8 and m.shape == (70, N.D) and set(np.unique(m)) <= {0, 1}
        want = np.array([[N.draw_mask16_int(SEED, 3, 1, r, col, keep) for col in range(N.D)] for r in range(70)], np.uint8)
        assert np.array_equal(m, want), keep
    big = N.draw_mask16(SEED, 3, 1, 4097, 0.9)
    assert abs(big.mean() - 0.9) < 0.01
    assert np.array_equal(big[:70], N.draw_mask16(SEED, 3, 1, 70, 0.9))
    assert N.draw_mask16(SEED, 3, 1, 4097, 1.0).all()
    assert not np.array_equal(big, N.draw_mask16(SEED, 4, 1, 4097, 0.9))
    assert not np.array_equal(big, N.draw_mask16(SEED, 3, 2, 4097, 0.9))
    assert np.all(np.abs(big.mean(0) - 0.9) < 0.03)                   # every column's own field: 4,097 draws, sd 0.0047


@pytest.mark.parametrize("n", N.ROWS)
def test_layer_inputs_hold_what_they_claim(n):
    """on the float32 restatement's ss, T1 and T2, at both keeps"""
    for kind in N.KINDS:
        c = N.layer_inputs(n, kind)
        assert c is N.layer_inputs(n, kind) and not c["S"].flags.writeable
        assert all(c[k].dtype == F4 for k in ("ego", "S", "Wg", "bg", "Wb", "bb", "d_out", "d_ego_next"))
        assert (kind == "biased") == bool(c["bg"].any() and c["bb"].any())
        zero_rows = N.zero_dout_rows(n)
        assert not c["d_out"][zero_rows].any()
        rest = np.setdiff1d(np.arange(n), zero_rows)
        assert np.all(np.abs(c["d_out"][rest]).max(1) > 0)
        for keep in N.KEEPS:
            T1, T2, z, ss, inv = N.layer_pre(*N.layer_args(c), keep)
            assert ss.dtype == F4 and np.all(np.isfinite(inv))
            if kind == "unbiased":
                assert not T1[N.ROW_ZERO_PRE].any() and not T2[N.ROW_ZERO_PRE].any() and c["mask"][N.ROW_ZERO_PRE].all()
                assert c["d_out"][N.ROW_ZERO_PRE].all()
            if n > N.ROW_MASKED:
                assert not z[N.ROW_MASKED].any() and ss[N.ROW_MASKED] == 0 and c["d_out"][N.ROW_MASKED].any()
            if n > N.ROW_TINY and kind == "unbiased":
                assert 1e-16 < ss[N.ROW_TINY] < 1e-13 and c["d_out"][N.ROW_TINY].all()
            assert np.all(ss[N.FIRST_PLAIN:] > 1e-6)                  # far from the floor 1e-12
            if n >= 63:
                assert len(zero_rows) > n // 2
                assert {0, 1, 2, 255} <= set(np.unique(c["mask"]))
                plain = slice(N.FIRST_PLAIN, None)
                assert (T1[plain] > 0).any() and (T1[plain] < 0).any() and (T2[plain] > 0).any() and (T2[plain] < 0).any()
                assert 0.85 < (c["mask"] != 0).mean() < 0.95


def test_marker_inputs_hold_one_row():
    for n, rows in N.MARKER_ROWS.items():
        assert n in N.ROWS and n - 1 in rows
        for r in rows:
            c = N.marker_inputs(n, r)
            live = np.flatnonzero(np.abs(c["d_out"]).max(1))
            assert live.tolist() == [r] and c["mask"][r].all()
            for k in ("d_out", "S", "ego"):
                assert np.all((np.abs(c[k][r]) >= 0.5) & (np.abs(c[k][r]) <= 1.5))
    assert N.MARKER_ROWS[65] == (0, 63, 64) and N.MARKER_ROWS[257] == (0, 63, 64, 256)
    assert N.MARKER_ROWS[4097] == (4095, 4096) and N.MARKER_ROWS[8200] == (4095, 4096, 8199)
