"""A numpy restatement of the width-generic dense kernels (csrc/ngcf_wide.hip: the row-wise NGCF kernels;
csrc/vae_wide.hip: the Mult-VAE pieces and the ordered column sums; csrc/gemm.hip: the split-K association and the
transpose) and the inputs the dense tests feed them.  Every function works in the dtype of its arrays: with float32
arrays it performs the operations in the order the kernel comments document, one rounding per operation (the library is
built with -ffp-contract=off: a + b * c is two roundings unless the kernel writes fmaf), and is the bit-exact
expectation wherever no device libm function is involved; with float64 arrays the same function is the high-precision
reference.  Hyper-parameters (keep, anneal, the constants 0.2 and 1e-12) are rounded to float32 first in both widths,
as the C ABI receives them.  The random draws are restated from the hash in Python integers.  Checked on the host in
test_dense_cpu.py; shared inputs are built once per case and handed out read-only."""
import functools

import numpy as np

from oracle import native

M64 = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15
NODE_SALT = 0x6e6f6465
LEAKY = np.float32(0.2)                   # kLeaky
NORM_EPS = np.float32(1e-12)              # kNormEps; also the floor under the item count of vae_bag_fwd
WAVE = 64
MAX_WIDTH = 256                           # 64 lanes x kMaxPer = 4 columns
RED_CHUNK = 32                            # kRedChunk of gemm.hip
KT = 16                                   # k rows per LDS tile of gemm.hip


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ------------------------------------------------------------------ arithmetic building blocks
def fmaf(a, b, c):
    """a * b + c with ONE rounding.  float64: the plain expression (the reference).  float32: the product of two
    float32 is exact in float64; the float64 sum is rounded to odd (its exact error comes from the two-sum), and a
    round-to-odd value of 53 bits rounds to the 24 bits of float32 as the exact sum would — no double rounding."""
    a, b, c = (np.asarray(x) for x in (a, b, c))
    if a.dtype == np.float64:
        return a * b + c
    assert a.dtype == b.dtype == c.dtype == np.float32, (a.dtype, b.dtype, c.dtype)
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = np.atleast_1d(p + c)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0)
    bits = bits + np.where(fix, np.where((err > 0) == (s > 0), 1, -1), 0)
    return bits.view(np.float64).astype(np.float32).reshape(np.broadcast(p, c).shape)


def tree_sum(v):
    """the halving tree over the last axis (a power of two): v = v[:n/2] + v[n/2:] down to 1.  With 64 entries it is
    nr_wave_sum_f32 (the xor butterfly x += shfl_xor(x, 32), 16, ..., 1: every lane ends with this sum), with 1,024 the
    LDS reduction of vae_softmax_dlogits_kernel (s_red[tid] += s_red[tid + s], s = 512 .. 1)"""
    n = v.shape[-1]
    assert n & (n - 1) == 0
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:]
    return v[..., 0]


def _lanes(x, width=WAVE):
    """[n][w] -> [n][ceil(w / width)][width]: lane l holds columns l, l + width, ...; columns past w are zeros"""
    n, w = x.shape
    q = -(-w // width)
    out = np.zeros((n, q * width), x.dtype)
    out[:, :w] = x
    return out.reshape(n, q, width)


def lrelu(x):
    return np.where(x > 0, x, x * x.dtype.type(LEAKY))


def act_fwd(act, x):
    """-1 / 3 identity, 0 tanh, 1 sigmoid as 1 / (1 + exp(-x)), 2 relu"""
    one = x.dtype.type(1)
    if act == 0:
        return np.tanh(x)
    if act == 1:
        return one / (one + np.exp(-x))
    if act == 2:
        return np.maximum(x, x.dtype.type(0))
    return x


def act_bwd(act, dY, Y):
    """nrhip_act_bwd: dY * act'(pre-activation) written from the output Y"""
    one = Y.dtype.type(1)
    if act == 0:
        return dY * (one - Y * Y)
    if act == 1:
        return dY * (Y * (one - Y))
    if act == 2:
        return dY * np.where(Y > 0, one, Y.dtype.type(0))
    return dY * one


# ------------------------------------------------------------------ the hash and the three draws
def splitmix64(x):
    x = (x + GOLDEN) & M64
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & M64
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def splitmix64_array(x):
    """the same on a uint64 array (wrapping arithmetic); pinned to the Python-integer form in test_dense_cpu.py"""
    with np.errstate(over="ignore"):
        x = x + np.uint64(GOLDEN)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return x ^ (x >> np.uint64(31))


def layer_mask_key(seed, step, layer):
    """ngcf_act_fwd / lrelu_drop_fwd: splitmix64(seed ^ (step * golden + layer))"""
    return splitmix64(seed ^ ((step * GOLDEN + layer) & M64))


def edge_mask_key(seed, step):
    return splitmix64(seed ^ ((step * GOLDEN + NODE_SALT) & M64))


def bag_drop_key(seed, step):
    return splitmix64(seed ^ ((step * GOLDEN) & M64))


def _hashes(key, n, first=0):
    return splitmix64_array(np.uint64(key) ^ (np.uint64(first) + np.arange(n, dtype=np.uint64)))


def draw_mask(key, n, keep):
    """element e is kept when (float)(splitmix64(key ^ e) >> 40) * 2^-24 < keep: 24 bits, exact in float32"""
    u = (_hashes(key, n) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u < np.float32(keep)).astype(np.uint8)


def uniform01(h):
    """vae_wide.hip: ((float)(h >> 40) + 0.5f) * 2^-24 — the + 0.5 is a float32 addition (it rounds above 2^23)"""
    return ((h >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def draw_bag_keep(key, n, keep):
    """vae_bag_fwd's dropout value per CSR position 0 .. n - 1: 1.0 when keep >= 1 or uniform01 < keep, else 0.0"""
    if np.float32(keep) >= 1:
        return np.ones(n, np.float32)
    return (uniform01(_hashes(key, n)) < np.float32(keep)).astype(np.float32)


def draw_eps(seed, step, batch, z, dtype):
    """vae_sample's Box-Muller draw N(0, 0.01^2): k0 = splitmix64(splitmix64(seed ^ 0xabcd ^ (step << 20)) ^ (r z + c)),
    u1 = uniform01(k0), u2 = uniform01(splitmix64(k0)), eps = 0.01 sqrt(-2 log u1) cos(6.2831853f u2) in `dtype`"""
    k0 = _hashes(splitmix64(seed ^ 0xabcd ^ ((step << 20) & M64)), batch * z)
    u1, u2 = uniform01(k0).astype(dtype), uniform01(splitmix64_array(k0)).astype(dtype)
    f = lambda x: dtype(np.float32(x))
    return ((f(0.01) * np.sqrt(f(-2.0) * np.log(u1))) * np.cos(f(6.2831853) * u2)).reshape(batch, z)


# ------------------------------------------------------------------ A. the NGCF row-wise kernels
def ew_mul(a, b):
    return a * b


def _row_sumsq(z):
    """per lane the fmaf chain over its columns q = 0 .. 3, then the wave sum"""
    Z = _lanes(z)
    ss = np.zeros((z.shape[0], WAVE), z.dtype)
    for q in range(Z.shape[1]):
        ss = fmaf(Z[:, q], Z[:, q], ss)
    return tree_sum(ss)


def _inv_norm(ss):
    dt = ss.dtype.type
    return dt(1) / np.sqrt(np.maximum(ss, dt(NORM_EPS)))


def ngcf_act_fwd(T1, T2, mask, keep, w_pad=None):
    """(E' [n][w_pad] with zero pad columns, l2_normalize(E') [n][w]):  Z = lrelu(T1) + lrelu(T2);
    E' = mask ? Z / keep : 0;  out = E' * (1 / sqrt(max(sum E'^2, 1e-12)))"""
    dt = T1.dtype.type
    n, w = T1.shape
    assert 1 <= w <= MAX_WIDTH
    zz = lrelu(T1) + lrelu(T2)
    z = np.where(mask != 0, zz / dt(np.float32(keep)), dt(0))
    out = z * _inv_norm(_row_sumsq(z))[:, None]
    ego = np.zeros((n, w if w_pad is None else w_pad), T1.dtype)
    ego[:, :w] = z
    return ego, out


def ngcf_act_bwd(d_out, d_ego_next, ego_next, T1, T2, mask, keep):
    """(dT1, dT2): with z = E', inv = 1 / sqrt(max(|z|^2, 1e-12)), dot = sum g (z inv) (lane fmaf chains, wave sum):
    v = |z|^2 > 1e-12 ? (g - (z inv) dot) inv : g inv;  v += d_ego_next;  dz = mask ? v / keep : 0;
    dT = T > 0 ? dz : dz * 0.2"""
    dt = T1.dtype.type
    ss = _row_sumsq(ego_next)
    inv = _inv_norm(ss)[:, None]
    G, Zi = _lanes(d_out), _lanes(ego_next * inv)
    dot = np.zeros((T1.shape[0], WAVE), T1.dtype)
    for q in range(G.shape[1]):
        dot = fmaf(G[:, q], Zi[:, q], dot)
    dot = tree_sum(dot)[:, None]
    v = np.where((ss > dt(NORM_EPS))[:, None], (d_out - (ego_next * inv) * dot) * inv, d_out * inv)
    if d_ego_next is not None:
        v = v + d_ego_next
    dz = np.where(mask != 0, v / dt(np.float32(keep)), dt(0))
    return np.where(T1 > 0, dz, dz * dt(LEAKY)), np.where(T2 > 0, dz, dz * dt(LEAKY))


def ngcf_mix_bwd(Y1, Y2, ego, S, w_pad):
    """(dS, d_ego_direct) [n][w_pad]: dS = Y1 + Y2 * ego (two roundings), d_ego_direct = Y2 * S; pad columns zero"""
    n, w = Y1.shape
    dS, dE = np.zeros((n, w_pad), Y1.dtype), np.zeros((n, w_pad), Y1.dtype)
    dS[:, :w] = Y1 + Y2 * ego
    dE[:, :w] = Y2 * S
    return dS, dE


def lrelu_drop_fwd(T, mask, keep, flags):
    """y = flags & 1 ? lrelu(T) : T;  flags & 2: y = mask ? y / keep : 0"""
    dt = T.dtype.type
    y = lrelu(T) if flags & 1 else T.copy()
    if flags & 2:
        y = np.where(mask != 0, y / dt(np.float32(keep)), dt(0))
    return y


def lrelu_drop_bwd(d_a, d_b, T, mask, keep, flags):
    dt = d_a.dtype.type
    g = d_a.copy() if d_b is None else d_a + d_b
    if flags & 2:
        g = np.where(mask != 0, g / dt(np.float32(keep)), dt(0))
    if flags & 1:
        g = np.where(T > 0, g, g * dt(LEAKY))
    return g


def edge_dropout(vals, kept, keep):
    """kept ? vals * (1 / keep) : 0 — the reciprocal is rounded before the product"""
    dt = vals.dtype.type
    return np.where(kept != 0, vals * (dt(1) / dt(np.float32(keep))), dt(0))


# ------------------------------------------------------------------ B. the Mult-VAE wide kernels
def vae_bag_fwd(indptr, indices, rows, W, bias, act, keep, kept):
    """(positions, h0val at them, Y before the activation, Y): per batch row the item count n, inv = 1 / sqrt(max(n,
    1e-12)), value (inv / keep) * kept[t] per CSR position t, and per output column the fmaf chain over the row's
    positions in ascending order from 0, + bias (one more rounding), then the activation.  kept: 0.0 / 1.0 per CSR
    position (given, or draw_bag_keep)."""
    dt = W.dtype.type
    pos, vals = [], []
    pre = np.zeros((len(rows), W.shape[1]), W.dtype)
    for r, u in enumerate(rows):
        b, e = int(indptr[u]), int(indptr[u + 1])
        inv = dt(1) / np.sqrt(np.maximum(dt(np.float32(e - b)), dt(NORM_EPS)))
        v = (inv / dt(np.float32(keep))) * kept[b:e].astype(W.dtype)
        acc = np.zeros(W.shape[1], W.dtype)
        for t in range(b, e):
            acc = fmaf(np.full(W.shape[1], v[t - b], W.dtype), W[indices[t]], acc)
        pre[r] = acc + bias
        pos.append(np.arange(b, e))
        vals.append(v)
    return np.concatenate(pos), np.concatenate(vals), pre, act_fwd(act, pre)


def vae_sample(H2, eps, is_training):
    """H2 = [mu | logvar] -> (EPSSTD, ZS, KLb): sd = exp(0.5 logvar); EPSSTD = eps sd; ZS = mu + is_training EPSSTD;
    KL term 0.5 (((-logvar + exp(logvar)) + mu mu) - 1), per lane added over its columns l, l + 64, ..., wave sum"""
    dt = H2.dtype.type
    z = H2.shape[1] // 2
    mu, logvar = H2[:, :z], H2[:, z:]
    es = eps * np.exp(dt(0.5) * logvar)
    term = dt(0.5) * (((-logvar + np.exp(logvar)) + mu * mu) - dt(1))
    T = _lanes(term)
    kl = np.zeros((H2.shape[0], WAVE), H2.dtype)
    for q in range(T.shape[1]):
        kl = kl + T[:, q]
    return es, mu + dt(np.float32(is_training)) * es, tree_sum(kl)


def vae_sample_bwd(dZ, H2, EPSSTD, anneal):
    """dH2 = [dZ + (anneal mu) / B  |  (dZ EPSSTD) 0.5 + ((anneal 0.5) (exp(logvar) - 1)) / B], 1 / B rounded first"""
    dt = H2.dtype.type
    batch, z = dZ.shape
    mu, logvar = H2[:, :z], H2[:, z:]
    a, invB = dt(np.float32(anneal)), dt(1) / dt(np.float32(batch))
    return np.concatenate([dZ + (a * mu) * invB,
                           (dZ * EPSSTD) * dt(0.5) + ((a * dt(0.5)) * (np.exp(logvar) - dt(1))) * invB], axis=1)


def _strided_sum(x, threads=1024):
    """thread t adds x[t], x[t + threads], ... in order from 0; then the halving tree over the threads"""
    X = _lanes(x[None, :], threads)[0]
    acc = np.zeros(threads, x.dtype)
    for q in range(X.shape[0]):
        acc = acc + X[q]
    return tree_sum(acc)


def softmax_dlogits(S, items, batch=None):
    """(nll [B], dlogits [B][cols]) of vae_softmax_dlogits_kernel: per row mx = max, sum = sum exp(x - mx) (1,024
    strided partial sums, halving tree), lse = mx + log(sum), nll = -sum over the row's items of (x_i - lse) (same
    reduction), dlogits = (exp(x - lse) n_b) (1 / B), minus 1 / B at the row's items.  items: one index array per row."""
    dt = S.dtype.type
    B = len(S) if batch is None else batch
    invB = dt(1) / dt(np.float32(B))
    nll, D = np.zeros(len(S), S.dtype), np.zeros_like(S)
    for r, row in enumerate(S):
        mx = row.max()
        lse = mx + np.log(_strided_sum(np.exp(row - mx)))
        it = np.asarray(items[r], np.int64)
        nll[r] = -_strided_sum(row[it] - lse)
        D[r] = (np.exp(row - lse) * dt(np.float32(len(it)))) * invB
        D[r, it] -= invB
    return nll, D


def dwq0_wide(indptr, indices, rows, h0val, DA1, dW):
    """dW[item] += h0val[t] * DA1[r] over the batch's CSR positions, in batch order (the device's atomics take any)"""
    for r, u in enumerate(rows):
        for t in range(int(indptr[u]), int(indptr[u + 1])):
            dW[indices[t]] = dW[indices[t]] + h0val[t] * DA1[r]
    return dW


def _colsum_block(X):
    """one block of colsum_rows_kernel: group g adds rows g, g + 16, ... in order from 0, then the 16 group sums are
    added in group order"""
    rows, cols = X.shape
    P = np.zeros((-(-max(rows, 1) // 16) * 16, cols), X.dtype)
    P[:rows] = X
    P = P.reshape(-1, 16, cols)
    acc = np.zeros((16, cols), X.dtype)
    for i in range(P.shape[0]):
        acc = acc + P[i]
    t = acc[0]
    for g in range(1, 16):
        t = t + acc[g]
    return t


def colsum_rows(X):
    """nrhip_colsum_rows: up to 2,048 rows one block; above, chunks of 512 rows summed the same way and the chunk sums
    — one row per chunk — summed by the same block once more"""
    if X.shape[0] <= 2048:
        return _colsum_block(X)
    return _colsum_block(np.stack([_colsum_block(X[r:r + 512]) for r in range(0, X.shape[0], 512)]))


# ------------------------------------------------------------------ C. the GEMM's associations
def fma_chain(A, B, C0=None):
    """C[m][n] = the k-ascending chain acc = fmaf(A[m][k], B[n][k], acc) from C0 (or 0): what gemm_lds_kernel computes,
    continued from C when it accumulates.  From 0 in float32 it is oracle.native.score_gemm (pinned in
    test_dense_cpu.py), which the split form below uses for speed."""
    acc = np.zeros((A.shape[0], B.shape[0]), A.dtype) if C0 is None else C0.copy()
    for k in range(A.shape[1]):
        acc = fmaf(np.broadcast_to(A[:, k, None], acc.shape), np.broadcast_to(B[None, :, k], acc.shape), acc)
    return acc


def _product(A, B):
    if A.dtype == np.float32:
        return native.score_gemm(np.ascontiguousarray(A), None, np.ascontiguousarray(B))
    return A @ B.T


def split_plan(K, splits):
    """(per, used) as nrhip_gemm_f32 cuts K: per = ceil(ceil(K / splits) / 16) * 16 k per part, used = ceil(K / per)"""
    per = -(-(-(-K // splits)) // KT) * KT
    return per, -(-K // per)


def gemm(A, B, splits=1, C0=None, bias=None, act=-1):
    """nrhip_gemm_f32 on A [M][K], B [N][K] (the contraction index last, as score_gemm takes them):
    splits = 1: the chain, continued from C0;  splits > 1: each part the chain of its k range from 0, the parts added
    left to right onto C0 (or 0) — with splits > 64 the parts are first summed in chunks of 32 (from 0, left to right)
    and the chunk sums added in order.  Then + bias[n], then the activation."""
    dt = A.dtype.type
    if splits == 1:
        acc = _product(A, B) if C0 is None else fma_chain(A, B, C0)
    else:
        per, used = split_plan(A.shape[1], splits)
        parts = [_product(A[:, s * per:(s + 1) * per], B[:, s * per:(s + 1) * per]) for s in range(used)]
        if splits > 2 * RED_CHUNK:
            chunks = []
            for c0 in range(0, used, RED_CHUNK):
                t = np.zeros_like(parts[0])
                for p in parts[c0:c0 + RED_CHUNK]:
                    t = t + p
                chunks.append(t)
            parts = chunks
        acc = np.zeros_like(parts[0]) if C0 is None else C0.copy()
        for p in parts:
            acc = acc + p
    if bias is not None:
        acc = acc + bias[None, :]
    return act_fwd(act, acc) if act >= 0 else acc


# ------------------------------------------------------------------ shared inputs
NGCF_WIDTHS = (1, 24, 63, 64, 65, 128, 129, 200, 256)
NGCF_ROWS = (1, 3, 4, 5, 1001)            # four rows share a block
NGCF_KEEPS = (1.0, 0.9)
ROW_ZERO, ROW_MASKED, ROW_TINY = 0, 1, 2  # the special rows of a case with at least 3 rows (row 0 alone: all-zero)


@functools.lru_cache(maxsize=None)
def ngcf_inputs(n, w):
    """T1, T2 (entries exactly 0 and negative ones among them), the gradients and forward tensors the backward kernels
    read, and a mask at keep 0.9.  Row 0 is all-zero in T1 and T2; with n >= 3 row 1 is fully masked out and row 2 has
    entries of size 1e-7 / sqrt(w) (a row of norm near 1e-7 at every width: its squared norm is below 1e-12, every
    other row's is 0 or far above)."""
    rs = np.random.RandomState(1000 * n + w)
    f = lambda *s: rs.randn(*s).astype(np.float32)
    T1, T2 = f(n, w), f(n, w)
    T1[rs.rand(n, w) < 0.1] = 0
    T2[rs.rand(n, w) < 0.1] = 0
    mask = (rs.rand(n, w) < 0.9).astype(np.uint8)
    T1[ROW_ZERO] = T2[ROW_ZERO] = 0
    if n >= 3:
        mask[ROW_MASKED] = 0
        T1[ROW_TINY] = 1e-7 * rs.randn(w) / np.sqrt(w)
        T2[ROW_TINY] = 1e-7 * rs.randn(w) / np.sqrt(w)
        mask[ROW_TINY] = 1
        mask[3:, 0] = 1                                     # an ordinary row keeps at least one entry
    out = {"T1": T1, "T2": T2, "mask": mask, "d_out": f(n, w), "d_ego_next": f(n, w), "Y1": f(n, w), "Y2": f(n, w),
           "ego": f(n, w), "S": f(n, w), "d_a": f(n, w), "d_b": f(n, w)}
    return _frozen(out)


BAG_ITEM_COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, 129)
BAG_ITEMS = 200


@functools.lru_cache(maxsize=None)
def bag_csr():
    """(indptr, indices, rows): 24 users over 200 items; the batch names 10 non-adjacent users with 0, 1, 7, 8, 9, 63,
    64, 65 and 129 items, one of them (the 9-item user) twice; the users between hold 5 items each and are not named"""
    rs = np.random.RandomState(11)
    counts = []
    for c in BAG_ITEM_COUNTS:
        counts += [5, c]
    counts += [5] * (24 - len(counts))
    indices = np.concatenate([np.sort(rs.choice(BAG_ITEMS, c, replace=False)) for c in counts]).astype(np.int32)
    indptr = np.r_[0, np.cumsum(counts)].astype(np.int64)
    users = 1 + 2 * np.arange(len(BAG_ITEM_COUNTS))
    rows = np.r_[users[::-1], users[4]].astype(np.int32)          # reversed: not ascending either
    for a in (indptr, indices, rows):
        a.setflags(write=False)
    return indptr, indices, rows


SOFTMAX_ITEM_COUNTS = (0, 1, 1023, 1024, 1025, 37)
SOFTMAX_PLAIN_ROW = 5


def softmax_case(cols):
    """(S [6][ld], item lists, ld): rows with 0, 1, 1023, 1024 and 1025 items where cols allows (else cols items at
    most), one logit near 80 in each of them and one of 95 in the third (without the max shift expf overflows there);
    a sixth row of ordinary logits, |x| <= 3, with 37 items, whose softmax spreads over all columns; ld = cols padded
    to 64 with the canary 7.0 in the pad"""
    rs = np.random.RandomState(cols)
    ld = (cols // 64 + 1) * 64
    counts = [min(c, cols) for c in SOFTMAX_ITEM_COUNTS]
    S = np.full((len(counts), ld), 7.0, np.float32)
    S[:, :cols] = np.clip(rs.randn(len(counts), cols), -3, 3)
    big = rs.randint(0, cols, 5)
    S[np.arange(5), big] = 80.0 + rs.rand(5)
    if cols > 1:
        S[2, (big[2] + 1) % cols] = 95.0                      # expf(80) = 5.5e34 is still finite: expf(95) is not
    items = [np.sort(rs.choice(cols, c, replace=False)).astype(np.int32) for c in counts]
    return S, items, ld
