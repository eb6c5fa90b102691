"""A numpy restatement of the narrow (d = 16) NGCF layer of csrc/dense.hip — ngcf_layer_fwd_quad_kernel,
ngcf_layer_bwd_quad_kernel and, in float64 only, the sums that ngcf_wgrad16_kernel / ngcf_wgrad_reduce_kernel form on the
matrix cores — and the inputs the layer tests feed them.  As in dense_restatement.py every function works in the dtype
of its arrays: with float32 arrays it performs the operations in the order dense.hip documents, one rounding per
operation (k-ascending fmaf chains from the bias, the SEQUENTIAL fmaf chain of the row's squared norm — four lanes own
a row and each of them walks all 16 columns, there is no lane tree here —, j-ascending chains for the transposed
products, everything else rounded on its own: the library is built with -ffp-contract=off), and is the bit-exact
expectation; with float64 arrays the same function is the reference.  keep, 0.2 and 1e-12 are rounded to float32 first
in both widths.  Checked on the host in test_ngcf_layer_cpu.py; shared inputs are built once per case, read-only."""
import functools

import numpy as np

from dense_restatement import LEAKY, NORM_EPS, fmaf, layer_mask_key, lrelu, splitmix64, splitmix64_array

D = 16
SLAB = 64                                  # rows per workgroup of the row kernels and per MFMA slab (kQuadRows, kWgradSlab)
SLAB_FLOATS = 544                          # 256 + 256 + 16 + 16 partial sums per slab
ROWS = (1, 3, 63, 64, 65, 255, 256, 257, 4096, 4097, 8200)
KEEPS = (1.0, 0.9)
KINDS = ("biased", "unbiased")
# the constructed rows (present when the case has that many rows)
ROW_ZERO_PRE, ROW_MASKED, ROW_TINY, FIRST_PLAIN = 0, 1, 2, 3


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _affine(x, W, b):
    """T[r][j]: from b[j], k = 0 .. 15 ascending, t = fmaf(x[r][k], W[k][j], t)   (quad_affine)"""
    t = np.broadcast_to(b.reshape(1, -1), (x.shape[0], W.shape[1])).astype(x.dtype)
    for k in range(W.shape[0]):
        t = fmaf(np.broadcast_to(x[:, k, None], t.shape), np.broadcast_to(W[None, k, :], t.shape), t)
    return t


def _affine_t(g, W):
    """y[r][i]: from 0, j = 0 .. 15 ascending, acc = fmaf(g[r][j], W[i][j], acc)   (quad_affine_t)"""
    acc = np.zeros((g.shape[0], W.shape[0]), g.dtype)
    for j in range(W.shape[1]):
        acc = fmaf(np.broadcast_to(g[:, j, None], acc.shape), np.broadcast_to(W[None, :, j], acc.shape), acc)
    return acc


def _row_chain(a, b):
    """per row from 0, k ascending: acc = fmaf(a[r][k], b[r][k], acc)"""
    acc = np.zeros(a.shape[0], a.dtype)
    for k in range(a.shape[1]):
        acc = fmaf(a[:, k], b[:, k], acc)
    return acc


def layer_pre(ego, S, Wg, bg, Wb, bb, mask, keep):
    """what both row kernels compute first: (T1, T2, z, ss, inv)"""
    dt = ego.dtype.type
    bi = ego * S                                                # __fmul_rn
    T1, T2 = _affine(S, Wg, bg.reshape(-1)), _affine(bi, Wb, bb.reshape(-1))
    zz = lrelu(T1) + lrelu(T2)
    z = np.where(mask != 0, zz / dt(np.float32(keep)), dt(0))
    ss = _row_chain(z, z)
    inv = dt(1) / np.sqrt(np.maximum(ss, dt(NORM_EPS)))
    return T1, T2, z, ss, inv


def layer_fwd(ego, S, Wg, bg, Wb, bb, mask, keep, pre=None):
    """(ego_out, out) = (z, z * inv); `pre`: a layer_pre result of the same arguments, to share it"""
    T1, T2, z, ss, inv = pre or layer_pre(ego, S, Wg, bg, Wb, bb, mask, keep)
    return z, z * inv[:, None]


def layer_bwd_rows(ego, S, Wg, bg, Wb, bb, mask, keep, d_out, d_ego_next, pre=None):
    """(dS, d_ego_direct, dT1, dT2): dot = the chain of g[k] * fl(z[k] inv);  v = ss > 1e-12 ? (g - (z inv) dot) inv :
    g inv;  v += d_ego_next when given;  dz = mask ? v / keep : 0;  dT = T > 0 ? dz : dz * 0.2;  y1 = dT1 Wg^T,
    y2 = dT2 Wb^T;  dS = y1 + fl(y2 * ego);  d_ego_direct = y2 * S"""
    dt = ego.dtype.type
    T1, T2, z, ss, inv = pre or layer_pre(ego, S, Wg, bg, Wb, bb, mask, keep)
    inv = inv[:, None]
    zi = z * inv
    dot = _row_chain(d_out, zi)[:, None]
    v = np.where((ss > dt(NORM_EPS))[:, None], (d_out - zi * dot) * inv, d_out * inv)
    if d_ego_next is not None:
        v = v + d_ego_next
    dz = np.where(mask != 0, v / dt(np.float32(keep)), dt(0))
    dT1, dT2 = np.where(T1 > 0, dz, dz * dt(LEAKY)), np.where(T2 > 0, dz, dz * dt(LEAKY))
    y1, y2 = _affine_t(dT1, Wg), _affine_t(dT2, Wb)
    return y1 + y2 * ego, y2 * S, dT1, dT2


def layer_wgrads(ego, S, dT1, dT2):
    """float64 only: ((dWg, dbg, dWb, dbb), (their sums of absolute terms)) with dWg = S^T dT1, dbg = sum_r dT1,
    dWb = (ego * S)^T dT2, dbb = sum_r dT2.  float32 ego and S are multiplied in float32 first (the kernel's
    __fmul_rn), then everything is float64; float64 ego and S are multiplied as they are."""
    f8 = lambda a: np.asarray(a, np.float64)
    bi = f8(ego * S) if ego.dtype == S.dtype else f8(ego) * f8(S)
    S, dT1, dT2 = f8(S), f8(dT1), f8(dT2)
    grads = (S.T @ dT1, dT1.sum(0), bi.T @ dT2, dT2.sum(0))
    terms = (np.abs(S).T @ np.abs(dT1), np.abs(dT1).sum(0), np.abs(bi).T @ np.abs(dT2), np.abs(dT2).sum(0))
    return grads, terms


WGRAD_ROUNDINGS = SLAB + 2
"""a slab's partial sum is at most 64 float32 accumulations (the bias sums: 16 additions and two shuffle steps), the
operand of dW_bi carries one more rounding, the combine over slabs is float64, the final cast one rounding"""


def wgrad_bound(terms):
    return WGRAD_ROUNDINGS * 2.0 ** -24 * np.asarray(terms, np.float64)


def draw_mask16(seed, step, layer, n_rows, keep):
    """uint8 [n_rows][16]: h = splitmix64(key ^ (r * 4 + q)) per (row, column quad); column 4 q + i is kept when
    float32((h >> 16 i) & 0xffff) * 2^-16 < float32(keep) — 16 bits per draw, not the 24 of the wide kernels"""
    key = layer_mask_key(seed, step, layer)
    h = splitmix64_array(np.uint64(key) ^ np.arange(n_rows * (D // 4), dtype=np.uint64))
    f = (h[:, None] >> (np.uint64(16) * np.arange(4, dtype=np.uint64))[None, :]) & np.uint64(0xffff)
    u = f.astype(np.float32) * np.float32(2.0 ** -16)
    return (u < np.float32(keep)).astype(np.uint8).reshape(n_rows, D)


def draw_mask16_int(seed, step, layer, r, c, keep):
    """one byte of the same in Python integers"""
    h = splitmix64(layer_mask_key(seed, step, layer) ^ (r * 4 + c // 4))
    return int(np.float32((h >> (16 * (c % 4))) & 0xffff) * np.float32(2.0 ** -16) < np.float32(keep))


def zero_dout_rows(n):
    """the rows of a case whose d_out is all zero: two of three from row 3 on (in a step most rows are outside the batch)"""
    r = np.arange(n)
    return r[(r >= FIRST_PLAIN) & (r % 3 != 0)]


@functools.lru_cache(maxsize=None)
def layer_inputs(n, kind):
    """ego, S, d_out, d_ego_next ~ N(0, 0.5^2) / N(0, 1), Wg, Wb ~ N(0, 0.2^2), bg, bb ~ N(0, 0.05^2) ("biased") or zero
    ("unbiased"), and a mask at keep 0.9 whose kept bytes are 1, 2 or 255.  The constructed rows, where n allows:
      row 0: kept entirely; "unbiased": S = 0, so that T1 = T2 = 0 exactly and the backward takes the 0.2 branch on
             both (with biases the row is an ordinary one: a one-row case has weight gradients other than zero);
      row 1: masked out entirely (z = 0, ss = 0);
      row 2: kept entirely; "unbiased": S of size 1e-7, so that |z| is about 1e-7 and 0 < ss < 1e-12 (with biases of
             0.05 no S makes the row small: there it is an ordinary row);
      rows 3 ..: ordinary rows that keep at least column 0; d_out = 0 in those with r % 3 != 0."""
    assert kind in KINDS
    rs = np.random.RandomState(16 * n + KINDS.index(kind))
    f = lambda scale, *s: (scale * rs.randn(*s)).astype(np.float32)
    ego, S, d_out, d_next = f(0.5, n, D), f(0.5, n, D), f(1.0, n, D), f(1.0, n, D)
    Wg, Wb = f(0.2, D, D), f(0.2, D, D)
    bg, bb = (f(0.05, D), f(0.05, D)) if kind == "biased" else (np.zeros(D, np.float32), np.zeros(D, np.float32))
    kept = rs.rand(n, D) < 0.9
    mask = np.where(kept, rs.choice(np.array([1, 1, 1, 2, 255], np.uint8), (n, D)), 0).astype(np.uint8)
    mask[FIRST_PLAIN:, 0] = 1
    mask[ROW_ZERO_PRE] = 1
    if kind == "unbiased":
        S[ROW_ZERO_PRE] = 0
    if n > ROW_MASKED:
        mask[ROW_MASKED] = 0
    if n > ROW_TINY:
        mask[ROW_TINY] = 255
        if kind == "unbiased":
            S[ROW_TINY] = (0.5e-7 * rs.randn(D)).astype(np.float32)
    d_out[zero_dout_rows(n)] = 0
    return _frozen({"ego": ego, "S": S, "Wg": Wg, "bg": bg, "Wb": Wb, "bb": bb, "mask": mask, "d_out": d_out,
                    "d_ego_next": d_next})


def layer_args(c, dtype=None):
    """(ego, S, Wg, bg, Wb, bb, mask) of a case, the floats in `dtype` when given"""
    cast = (lambda a: a) if dtype is None else (lambda a: a.astype(dtype))
    return tuple(cast(c[k]) for k in ("ego", "S", "Wg", "bg", "Wb", "bb")) + (c["mask"],)


@functools.lru_cache(maxsize=None)
def marker_inputs(n, r):
    """layer_inputs(n, "biased") with d_out zero everywhere except row r; d_out[r], S[r] and ego[r] have entries of
    size 0.5 .. 1.5 with random signs and row r is kept entirely: every weight gradient is one outer product of row r"""
    assert 0 <= r < n
    c = {k: np.array(v) for k, v in layer_inputs(n, "biased").items()}
    rs = np.random.RandomState(100003 * n + r)
    one = lambda: (rs.uniform(0.5, 1.5, D) * rs.choice([-1.0, 1.0], D)).astype(np.float32)
    c["d_out"][:] = 0
    c["d_out"][r], c["S"][r], c["ego"][r] = one(), one(), one()
    c["mask"][r] = 1
    return _frozen(c)


MARKER_ROWS = {n: tuple(sorted({0, 63, 64, n - 1} if n < 4096 else {4095, 4096, n - 1})) for n in (65, 257, 4097, 8200)}
"""the first and last row of a slab on both sides of a slab edge, and of the 64-slab edge of the reduce loop"""
