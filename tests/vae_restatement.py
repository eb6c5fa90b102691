"""A numpy restatement of the narrow Mult-VAE kernels (csrc/vae.hip: the encoder, add_row_bias, the middle of the
backward pass with its three small weight gradients, the dW_q0 scatter; csrc/vae_fused.hip and the slab decoder of
vae.hip: the decoder's loss and gradients) and the frozen inputs the tests feed them.  Every function works in the dtype
it is given: in float32 it performs the operations in the order the kernel comments document, one rounding per
operation (the library is built with -ffp-contract=off: a + b * c is two roundings unless the kernel writes fmaf), and
is the bit-exact expectation wherever no device libm function is involved; in float64 the same function is the plain
formula, the high-precision reference.  The two decoders reassociate their sums (matrix-core tiles, per-workgroup
partials), so the float32 decoder here is only the yardstick: the same formulas in float32 with numpy's own sum order.
Hyper-parameters (keep, anneal, is_training) are rounded to float32 first in both widths, as the C ABI receives them.
Checked on the host in test_vae_cpu.py; shared inputs are built once per case and handed out read-only."""
import functools

import numpy as np

from dense_restatement import (WAVE, NORM_EPS, _frozen, _lanes, act_bwd, act_fwd, bag_drop_key, draw_bag_keep,
                               draw_eps, fma_chain, fmaf, splitmix64, tree_sum, uniform01)   # noqa: F401

ACTS = {"tanh": 0, "sigmoid": 1, "relu": 2, "identity": 3}
ENC_SEG, ENC_MAX_SEG = 256, 64            # kEncSeg, kEncMaxSeg of vae_encode_kernel
DWQ0_ROUND = 64 * 16                      # 4 waves x kDwq0SlotsY chunk slots x kDwq0Chunk items: one round of vae_dwq0
SEED = 2018


# ------------------------------------------------------------------ the device draws
def keep_mask(seed, step, nnz, keep):
    """vae_encode_kernel's dropout value per CSR position t = 0 .. nnz - 1: drop_key = splitmix64(seed ^ step *
    0x9e3779b97f4a7c15); kept when keep >= 1 or uniform01(splitmix64(drop_key ^ t)) < keep"""
    return draw_bag_keep(bag_drop_key(seed, step), nnz, keep)


def noise(seed, step, batch, z, dtype):
    """the Box-Muller draw as the kernel keys it: k0 = splitmix64(splitmix64(seed ^ 0xabcd ^ (step << 20)) ^ (r z +
    lane)), u1 = uniform01(k0), u2 = uniform01(splitmix64(k0)), eps = (0.01 sqrt(-2 log u1)) cos(6.2831853f u2)"""
    return draw_eps(seed, step, batch, z, dtype)


# ------------------------------------------------------------------ the encoder
def seg_plan(n):
    """(seg_len, n_seg) of a row of n items: segments of 256 items, merged into 64 longer ones above 16,384"""
    seg_len = max(ENC_SEG, -(-n // ENC_MAX_SEG))
    return seg_len, max(1, -(-n // seg_len))


def h0_values(indptr, kept, keep, dtype):
    """(inv / keep) * kept[t] per CSR position of EVERY row, inv = 1 / sqrt(max(n, 1e-12)) of the position's row"""
    dt = dtype
    n = np.diff(indptr)
    inv = dt(1) / np.sqrt(np.maximum(n.astype(np.float32).astype(dt), dt(NORM_EPS)))
    return np.repeat(inv / dt(np.float32(keep)), n) * kept.astype(dt)


def bag_sums(indptr, indices, rows, Wq0, vals, segmented=True):
    """a1 [B][h]: per segment of a row the fmaf chain over its positions in ascending order from 0, the segment sums
    added in segment order (segmented=False: one chain over the whole row).  All segments advance together here: step
    s of every chain is one vectorised fmaf."""
    segs, owner = [], []
    for r, u in enumerate(rows):
        b, e = int(indptr[u]), int(indptr[u + 1])
        seg_len, n_seg = seg_plan(e - b) if segmented else (max(e - b, 1), 1)
        for sg in range(n_seg):
            segs.append((b + sg * seg_len, min(e, b + (sg + 1) * seg_len)))
            owner.append(r)
    L = max(max(se - sb for sb, se in segs), 1)
    pos = np.full((len(segs), L), -1, np.int64)
    for i, (sb, se) in enumerate(segs):
        pos[i, :se - sb] = np.arange(sb, se)
    acc = np.zeros((len(segs), Wq0.shape[1]), Wq0.dtype)
    for s in range(L):
        live = np.nonzero(pos[:, s] >= 0)[0]
        if not len(live):
            break
        t = pos[live, s]
        acc[live] = fmaf(np.broadcast_to(vals[t][:, None], (len(t), Wq0.shape[1])), Wq0[indices[t]], acc[live])
    a1 = np.zeros((len(rows), Wq0.shape[1]), Wq0.dtype)
    first = np.ones(len(rows), bool)
    for i, r in enumerate(owner):                                  # segment order within a row
        a1[r] = acc[i] if first[r] else a1[r] + acc[i]
        first[r] = False
    return a1


def encode(indptr, indices, rows, P, act, keep, kept, eps, is_training, dtype, a1=None):
    """vae_encode_kernel: -> dict(pos, h0val (at pos), H1, MU, LOGVAR, EPSSTD, ZS, G1, KLb).  P: the float32 parameters
    (Wq0 [I][h], bq0, Wq1 [h][2z], bq1, Wp0 [z][h], bp0), converted to `dtype`; kept: 0 / 1 per CSR position; eps
    [B][z]; a1: bag_sums of the same inputs when the caller holds it already (it depends on neither act nor z)."""
    dt = dtype
    f = lambda x: np.asarray(x).astype(dt)
    Wq0, bq0, Wq1, bq1, Wp0, bp0 = (f(P[k]) for k in ("Wq0", "bq0", "Wq1", "bq1", "Wp0", "bp0"))
    h, z = Wq0.shape[1], Wp0.shape[0]
    vals = h0_values(indptr, kept, keep, dt)
    pos = np.concatenate([np.arange(indptr[u], indptr[u + 1]) for u in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    if a1 is None:
        a1 = bag_sums(indptr, indices, rows, Wq0, vals)
    B = len(rows)
    H1 = act_fwd(act, a1 + bq0[None, :])
    h2 = np.broadcast_to(bq1[None, :], (B, 2 * z)).copy()
    for k in range(h):
        h2 = fmaf(np.broadcast_to(H1[:, k, None], h2.shape), np.broadcast_to(Wq1[None, k, :], h2.shape), h2)
    mu, logvar = h2[:, :z], h2[:, z:]
    sd = np.exp(dt(0.5) * logvar)
    es = f(eps) * sd
    zs = mu + dt(np.float32(is_training)) * es
    term = dt(0.5) * ((((-logvar) + np.exp(logvar)) + mu * mu) - dt(1))
    klb = tree_sum(_lanes(term)[:, 0, :])                          # lanes >= z hold 0; z <= 16 is one lane column
    a3 = np.broadcast_to(bp0[None, :], (B, h)).copy()
    for k in range(z):
        a3 = fmaf(np.broadcast_to(zs[:, k, None], a3.shape), np.broadcast_to(Wp0[None, k, :], a3.shape), a3)
    return {"pos": pos, "h0val": vals[pos], "A1": a1, "H1": H1, "MU": mu.copy(), "LOGVAR": logvar.copy(), "EPSSTD": es,
            "ZS": zs, "G1": act_fwd(act, a3), "KLb": klb}


def add_row_bias(S, bias):
    return S + bias[None, :]


# ------------------------------------------------------------------ the decoder
def dense_rows(indptr, indices, rows, n_items, dtype):
    X = np.zeros((len(rows), n_items), dtype)
    for r, u in enumerate(rows):
        X[r, indices[indptr[u]:indptr[u + 1]]] = 1
    return X


def decoder_logits(G1, Wp1t, bp1):
    """the k-ascending fmaf chain from 0, then fmaf(1, b, dot) = dot + b rounded once"""
    return fma_chain(G1, Wp1t) + bp1[None, :]


def decoder(indptr, indices, rows, G1, Wp1t, bp1, dtype):
    """the header of vae_fused.hip: logits = g1 W_p1^T + b; lse; nll_b = -sum over the row's items of (logit - lse);
    G = (softmax n_b - x) / B; dW_p1 = G^T g1 [I][h]; db_p1 = colsum(G); dg1 = G W_p1 [B][h].  float64: the reference;
    float32: the same lines with numpy's sum order (the yardstick).  -> dict(logits, lse, nll, G, dWp1, dbp1, dg1)"""
    dt = dtype
    G1, W, b = (np.asarray(x).astype(dt) for x in (G1, Wp1t, bp1))
    B, I = len(rows), W.shape[0]
    logits = decoder_logits(G1, W, b)
    X = dense_rows(indptr, indices, rows, I, dt)
    mx = logits.max(axis=1, keepdims=True)
    lse = mx + np.log(np.sum(np.exp(logits - mx), axis=1, keepdims=True))
    nll = -np.sum((logits - lse) * X, axis=1)
    n_b = X.sum(axis=1, keepdims=True)
    G = (np.exp(logits - lse) * n_b - X) / dt(np.float32(B))
    return {"logits": logits, "lse": lse[:, 0], "nll": nll, "G": G, "dWp1": G.T @ G1, "dbp1": G.sum(axis=0),
            "dg1": G @ W}


# ------------------------------------------------------------------ the middle of the backward pass
def mid_backward(dG1, G1, H1, MU, LOGVAR, EPSSTD, Wp0, Wq1, act, anneal):
    """vae_mid_bwd_kernel line by line -> (DA3 [B][h], DH2 [B][2z], DA1 [B][h]):
    da3 = dg1 act'(g1);  dz[k] = the j-ascending fmaf chain of da3[j] W_p0[k][j] from 0;
    dmu = dz + (anneal mu) (1 / B);  dlogvar = (dz es) 0.5 + ((anneal 0.5) (exp(logvar) - 1)) (1 / B);
    da1 = (the j-ascending fmaf chain of dh2[j] W_q1[lane][j] from 0) act'(h1)"""
    dt = dG1.dtype.type
    B, h = dG1.shape
    z = MU.shape[1]
    a, invB = dt(np.float32(anneal)), dt(np.float32(1) / np.float32(B))
    DA3 = act_bwd(act, dG1, G1)
    dz = np.zeros((B, z), dG1.dtype)
    for j in range(h):
        dz = fmaf(np.broadcast_to(DA3[:, j, None], dz.shape), np.broadcast_to(Wp0[None, :, j], dz.shape), dz)
    dmu = dz + (a * MU) * invB
    dlv = (dz * EPSSTD) * dt(0.5) + ((a * dt(0.5)) * (np.exp(LOGVAR) - dt(1))) * invB
    DH2 = np.concatenate([dmu, dlv], axis=1)
    acc = np.zeros((B, h), dG1.dtype)
    for j in range(2 * z):
        acc = fmaf(np.broadcast_to(DH2[:, j, None], acc.shape), np.broadcast_to(Wq1[None, :, j], acc.shape), acc)
    return DA3, DH2, act_bwd(act, acc, H1)


def small_wgrad(X, G):
    """vae_small_wgrad3_kernel, one wave per output element: (dW [K][J], db [J]); lane l takes batch rows l, l + 64,
    ... in order — an fmaf chain of X[b][k] G[b][j] from 0 for dW, a plain sum of G[b][j] for db — then the wave sum.
    X None: the bias sum alone."""
    B, J = G.shape
    q = -(-B // WAVE)
    Gp = np.zeros((q * WAVE, J), G.dtype)
    Gp[:B] = G
    Gp = Gp.reshape(q, WAVE, J)
    db = np.zeros((WAVE, J), G.dtype)
    for i in range(q):
        db = db + Gp[i]
    db = tree_sum(db.T)
    if X is None:
        return None, db
    K = X.shape[1]
    Xp = np.zeros((q * WAVE, K), X.dtype)
    Xp[:B] = X
    Xp = Xp.reshape(q, WAVE, K)
    acc = np.zeros((K, J, WAVE), G.dtype)
    live = np.arange(q * WAVE).reshape(q, WAVE) < B
    for i in range(q):
        new = fmaf(np.broadcast_to(Xp[i].T[:, None, :], acc.shape), np.broadcast_to(Gp[i].T[None, :, :], acc.shape), acc)
        acc = np.where(live[i][None, None, :], new, acc)
    return tree_sum(acc), db


def mid_wgrads(ZS, H1, DA3, DH2, DA1):
    """(dWp0 [z][h], dbp0, dWq1 [h][2z], dbq1, dbq0) from the given DA3 / DH2 / DA1"""
    dWp0, dbp0 = small_wgrad(ZS, DA3)
    dWq1, dbq1 = small_wgrad(H1, DH2)
    return dWp0, dbp0, dWq1, dbq1, small_wgrad(None, DA1)[1]


def dwq0(indptr, indices, rows, h0val, DA1, n_items):
    """dW_q0 [I][h]: += h0val[t] DA1[r] (the product rounded, then added) over the batch's CSR positions, in batch
    order — np.add.at; the device's atomics take any order.  h0val: per CSR position of the whole matrix."""
    dW = np.zeros((n_items, DA1.shape[1]), DA1.dtype)
    for r, u in enumerate(rows):
        b, e = int(indptr[u]), int(indptr[u + 1])
        np.add.at(dW, indices[b:e], h0val[b:e, None] * DA1[r][None, :])
    return dW


# ------------------------------------------------------------------ frozen cases
BAG_ITEMS = 16500
BAG_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1040, 16384, 16385, 16500)
WIDTHS = ((32, 16), (20, 5), (31, 16), (32, 1), (5, 16), (1, 1))
SHORT = 257                               # "short" users: at most this many items
DRAWN_SIZES = (3, 4, 5, 63, 64, 65, 130)


def user_of(length):
    return BAG_LENGTHS.index(length)


@functools.lru_cache(maxsize=None)
def bag_csr():
    """(indptr, indices): user u holds BAG_LENGTHS[u] random items of 16,500, ascending"""
    rs = np.random.RandomState(31)
    indices = np.concatenate([np.sort(rs.choice(BAG_ITEMS, c, replace=False)) for c in BAG_LENGTHS]).astype(np.int32)
    indptr = np.r_[0, np.cumsum(BAG_LENGTHS)].astype(np.int64)
    indptr.setflags(write=False)
    indices.setflags(write=False)
    return indptr, indices


@functools.lru_cache(maxsize=None)
def batches():
    """name -> int32 user rows: `all` (every user, shuffled: the long rows), `repeat` (a user listed twice, next to
    the 1,025-item user), `single`, and b3 .. b130 drawn (with replacement above 15 rows: 15 users qualify) from the
    users of at most 257 items"""
    rs = np.random.RandomState(32)
    short = np.array([u for u, c in enumerate(BAG_LENGTHS) if c <= SHORT])
    out = {"all": rs.permutation(len(BAG_LENGTHS)),
           "repeat": np.array([user_of(c) for c in (17, 1025, 0, 64, 17, 33)]),
           "single": np.array([user_of(65)])}
    for n in DRAWN_SIZES:
        out["b%d" % n] = rs.choice(short, n, replace=n > len(short))
    out = {k: v.astype(np.int32) for k, v in out.items()}
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def params(h, z, n_items=BAG_ITEMS, seed=0):
    """weights 0.3 randn, biases 0.05 randn (tests/test_multivae_gpu.py::_problem)"""
    rs = np.random.RandomState(1000 * h + 10 * z + seed)
    w, b = (lambda *s: (rs.randn(*s) * 0.3).astype(np.float32)), (lambda n: (rs.randn(n) * 0.05).astype(np.float32))
    return _frozen({"Wq0": w(n_items, h), "bq0": b(h), "Wq1": w(h, 2 * z), "bq1": b(2 * z), "Wp0": w(z, h),
                    "bp0": b(h), "Wp1t": w(n_items, h), "bp1": b(n_items)})


@functools.lru_cache(maxsize=None)
def given_draws(z):
    """(kept per CSR position at keep 0.8, eps [22 + 130][z] ~ N(0, 0.01^2)): the masks / noise handed to the kernel"""
    rs = np.random.RandomState(33 + z)
    kept = (rs.rand(int(bag_csr()[0][-1])) < 0.8).astype(np.float32)
    eps = (rs.randn(160, z) * 0.01).astype(np.float32)
    kept.setflags(write=False)
    eps.setflags(write=False)
    return kept, eps


@functools.lru_cache(maxsize=None)
def encode_case(h, z, batch, act, keep, is_training, dtype):
    """encode() of a frozen case with the given draws (keep 1: nothing dropped); the bag sums are shared by the
    activations"""
    indptr, indices = bag_csr()
    rows = batches()[batch]
    kept, eps = given_draws(z)
    if keep >= 1:
        kept = np.ones_like(kept)
    a1 = _bag_sums_case(h, z, batch, keep, dtype)
    return _frozen(encode(indptr, indices, rows, params(h, z), ACTS[act], keep, kept, eps[:len(rows)], is_training,
                          dtype, a1=a1))


@functools.lru_cache(maxsize=None)
def _bag_sums_case(h, z, batch, keep, dtype):
    indptr, indices = bag_csr()
    kept = given_draws(z)[0] if keep < 1 else np.ones(int(indptr[-1]), np.float32)
    a1 = bag_sums(indptr, indices, batches()[batch], params(h, z)["Wq0"].astype(dtype),
                  h0_values(indptr, kept, keep, dtype))
    a1.setflags(write=False)
    return a1


MID_BATCHES = (1, 3, 4, 5, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def mid_inputs(B, h, z, act):
    """what nrhip_vae_mid_backward reads: dG1 (1 / B sized, as the decoder leaves it), G1 and H1 as outputs of the
    activation (relu: zeros among them), MU, LOGVAR, EPSSTD, ZS, and the two weight matrices"""
    rs = np.random.RandomState(7 * B + 100 * h + z + 1000 * ACTS[act])
    f = lambda *s: rs.randn(*s).astype(np.float32)
    p = params(h, z)
    return _frozen({"dG1": f(B, h) / np.float32(B), "G1": act_fwd(ACTS[act], f(B, h)), "H1": act_fwd(ACTS[act], f(B, h)),
                    "MU": f(B, z) * np.float32(0.5), "LOGVAR": f(B, z) * np.float32(0.5),
                    "EPSSTD": f(B, z) * np.float32(0.01), "ZS": f(B, z) * np.float32(0.5), "Wp0": p["Wp0"],
                    "Wq1": p["Wq1"]})


DEC_KINDS = ("unit", "wide", "flat", "buried")
DEC_FLAT_BIAS = np.float32(0.25)
DEC_POW2 = (1, 2, 4, 8, 16)               # flat rows read lse back through nll / n_b: exact when n_b is a power of two
WIDE_RANGE = 130.0
BURIED_LIFT = 45.0


@functools.lru_cache(maxsize=None)
def decoder_case(B, I, h, kind):
    """-> dict(indptr, indices, rows, G1 [B][h], W [I][h], b [I], hot).  Users: 0 has no history, 1 holds every item,
    2 .. 6 hold 1, 2, 4, 8, 16 items (as I allows), the others 1 .. 40 random ones; with I >= 31 two `hot` items (in
    the first and the last 32-item tile) belong to no user but user 1.  rows: B users — users 0 and 1 among them from
    B = 3 on, and from B = 4 on one user twice — shuffled.
    unit: G1 0.7 randn, W 0.5 randn, b 0.3 randn (tests/test_multivae_gpu.py);  wide: each row of G1 scaled so that
    its logits span 130;  flat: W = 0 and b = 0.25, every logit 0.25 and lse = 0.25 + log I;  buried: b += 45 on the hot
    items and user 1 replaced in the batch, so every positive lies at least 30 under its row's maximum."""
    rs = np.random.RandomState(B + 3 * I + h)
    n_users = B + 8
    hot = np.array([3, I - 2]) if I >= 31 else np.zeros(0, np.int64)
    cold = np.setdiff1d(np.arange(I), hot)
    counts = [0, I] + [min(c, len(cold)) for c in DEC_POW2]
    counts += [int(rs.randint(1, min(len(cold), 40) + 1)) for _ in range(n_users - len(counts))]
    lists = [np.zeros(0, np.int64), np.arange(I)] + [np.sort(rs.choice(cold, c, replace=False)) for c in counts[2:]]
    indptr = np.r_[0, np.cumsum(counts)].astype(np.int64)
    indices = np.concatenate(lists).astype(np.int32)
    full = 1 if kind != "buried" else 7
    if B == 1:
        rows = np.array([full])
    elif B == 2:
        rows = np.array([full, 0])
    else:
        rest = rs.permutation(np.arange(2, n_users))
        rest = rest[rest != full]
        rows = np.r_[0, full, rest[:B - 2]]
        if B >= 4:
            rows[-1] = rows[2]
        rows = rs.permutation(rows)
    G1 = (rs.randn(B, h) * 0.7).astype(np.float32)
    W = (rs.randn(I, h) * 0.5).astype(np.float32)
    b = (rs.randn(I) * 0.3).astype(np.float32)
    if kind == "wide" and I > 1:
        L = G1.astype(np.float64) @ W.astype(np.float64).T
        span = L.max(axis=1) - L.min(axis=1)
        G1 = (G1 * (WIDE_RANGE / np.maximum(span, 1e-3))[:, None]).astype(np.float32)
    if kind == "flat":
        W = np.zeros_like(W)
        b = np.full(I, DEC_FLAT_BIAS, np.float32)
    if kind == "buried":
        b[hot] += np.float32(BURIED_LIFT)
    return _frozen({"indptr": indptr, "indices": indices, "rows": rows.astype(np.int32), "G1": G1, "W": W, "b": b,
                    "hot": hot})


@functools.lru_cache(maxsize=None)
def decoder_want(B, I, h, kind, dtype):
    c = decoder_case(B, I, h, kind)
    return _frozen(decoder(c["indptr"], c["indices"], c["rows"], c["G1"], c["W"], c["b"], dtype))
