"""JCA restated in numpy, dtype-generic (float32 / float64): the block step of model/general_recommender/JCA.py as
neurec_amd/jca.py states it, the device's draw rule (csrc/jca.hip) and the scorer.  Dense on purpose: it forms the
[Bu, I] and [U, Bi] slabs the device code avoids.

    hu = g(R[r,:] UV + Ub1);  hi = g((R[:,c]^T IV + Ib1) * IF[c]);  D = (f(hu UW[:,c] + Ub2[c]) + f(hi IW[:,r] + Ib2[r])^T) / 2
    cost = sum over pairs max(0, D[a,bn] - D[a,bp] + margin) + reg * 0.5 * sum over the eight tables of sum(w^2) / 2
A pair is active when its hinge argument is > 0.  Adam in TensorFlow's form (lr_t, epsilon outside the root), dense on
every variable; `gd` is plain gradient descent.
"""
import numpy as np

from cdae_restatement import M64, XorShift64s, splitmix64

NAMES = ("UV", "UW", "Ub1", "Ub2", "IV", "IW", "Ib1", "Ib2", "I_factor_vector")      # the reference's creation order
REGULARISED = ("UW", "UV", "IW", "IV", "Ib1", "Ib2", "Ub1", "Ub2")
MAX_REJECTS = 64

# case -> (f_act, g_act, learner, reg, num_neg, H, margin, lr)
CASES = {
    "default": ("tanh", "tanh", "adam", 0.0, 1, 33, 0.15, 0.001),
    "gdreg": ("sigmoid", "relu", "gd", 0.05, 1, 16, 0.15, 0.05),
    "neg2": ("identity", "elu", "adam", 0.0, 2, 9, 0.15, 0.001),
}
EPOCH_CASE, EPOCH_BATCH, EPOCH_H = "default", 48, 50        # the epoch runs `default` at the reference's H


def shapes(U, I, H):
    return {"UV": (I, H), "UW": (H, I), "Ub1": (1, H), "Ub2": (1, I), "IV": (U, H), "IW": (H, U), "Ib1": (1, H),
            "Ib2": (1, U), "I_factor_vector": (1, I)}


def init_tables(U, I, H, seed, scale=0.1):
    """float32 tables in the creation order; larger than the reference's stddev of 0.01 so that the activations bend,
    and I_factor_vector around 1 so that the item encoder is alive"""
    rs = np.random.RandomState(seed)
    out = {}
    for k in NAMES:
        out[k] = (scale * rs.standard_normal(shapes(U, I, H)[k])).astype(np.float32)
    out["I_factor_vector"] = (1.0 + out["I_factor_vector"]).astype(np.float32)
    return out


def act(kind, x):
    if kind == "sigmoid":
        return 1 / (1 + np.exp(-x))
    if kind == "tanh":
        return np.tanh(x)
    if kind == "relu":
        return np.maximum(x, 0)
    if kind == "elu":
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    if kind == "identity":
        return x
    raise NotImplementedError(kind)


def dact(kind, y):
    """the derivative from the OUTPUT y"""
    one = y.dtype.type(1)
    if kind == "sigmoid":
        return y * (one - y)
    if kind == "tanh":
        return one - y * y
    if kind == "relu":
        return (y > 0).astype(y.dtype)
    if kind == "elu":
        return np.where(y > 0, one, y + one)
    return np.ones_like(y)


def forward(T, R, rows, cols, f, g):
    """(hu [Bu, H], pi, hi [Bi, H], Yu, Yi [Bu, Bi]); R dense [U, I] in the tables' dtype"""
    hu = act(g, R[rows] @ T["UV"] + T["Ub1"])
    pi = R[:, cols].T @ T["IV"] + T["Ib1"]
    hi = act(g, pi * T["I_factor_vector"][0, cols][:, None])
    Yu = act(f, hu @ T["UW"][:, cols] + T["Ub2"][0, cols][None, :])
    Yi = act(f, (hi @ T["IW"][:, rows] + T["Ib2"][0, rows][None, :]).T)
    return hu, pi, hi, Yu, Yi


def gradients(T, R, rows, cols, pairs, f, g, margin, reg):
    """-> (hinge term, regulariser term, {name: gradient WITHOUT the regulariser's 0.5 reg w}); pairs = (a, bp, bn)"""
    dt = T["UV"].dtype.type
    a, bp, bn = (np.asarray(x, np.int64) for x in pairs)
    hu, pi, hi, Yu, Yi = forward(T, R, rows, cols, f, g)
    D = (Yu + Yi) * dt(0.5)
    x = (D[a, bn] - D[a, bp]) + dt(margin)
    on = x > 0
    hinge = x[on].astype(np.float64).sum()
    cnt = np.zeros(D.shape, np.int64)
    np.add.at(cnt, (a[on], bn[on]), 1)
    np.add.at(cnt, (a[on], bp[on]), -1)
    half = cnt.astype(D.dtype) * dt(0.5)
    dxu, dxi = half * dact(f, Yu), half * dact(f, Yi)
    G = {k: np.zeros_like(v) for k, v in T.items()}
    G["UW"][:, cols] = hu.T @ dxu
    G["Ub2"][0, cols] = dxu.sum(0)
    G["IW"][:, rows] = hi.T @ dxi.T
    G["Ib2"][0, rows] = dxi.sum(1)
    dpu = (dxu @ T["UW"][:, cols].T) * dact(g, hu)
    dzi = (dxi.T @ T["IW"][:, rows].T) * dact(g, hi)
    G["I_factor_vector"][0, cols] = (dzi * pi).sum(1)
    dpi = dzi * T["I_factor_vector"][0, cols][:, None]
    G["Ub1"][0] = dpu.sum(0)
    G["Ib1"][0] = dpi.sum(0)
    G["UV"] = R[rows].T @ dpu
    G["IV"] = R[:, cols] @ dpi
    sq = sum(float((T[k].astype(np.float64) ** 2).sum()) for k in REGULARISED)
    return hinge, float(reg) * 0.25 * sq, G


class State:
    """the tables in `dtype` with TensorFlow's Adam slots and beta powers"""

    def __init__(self, tables, dtype, lr, learner="adam", beta1=0.9, beta2=0.999, eps=1e-8):
        t = np.dtype(dtype).type
        self.T = {k: np.array(tables[k], dtype=dtype) for k in NAMES}
        self.m = {k: np.zeros_like(v) for k, v in self.T.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.T.items()}
        self.t, self.lr, self.b1, self.b2, self.eps, self.learner = t, t(lr), t(beta1), t(beta2), t(eps), learner
        self.b1p, self.b2p = t(beta1), t(beta2)
        self.steps = 0


def step(st, R, rows, cols, pairs, f, g, margin, reg):
    """one block step -> (hinge term, regulariser term) before the update; no pair: nothing moves"""
    if len(pairs[0]) == 0:
        return 0.0, 0.0
    t = st.t
    hinge, regl, G = gradients(st.T, R, rows, cols, pairs, f, g, margin, reg)
    one, half_reg = t(1), t(0.5) * t(reg)
    lr_t = st.lr * np.sqrt(one - st.b2p) / (one - st.b1p)
    for k in NAMES:
        gk = G[k] + half_reg * st.T[k] if k in REGULARISED else G[k]
        if st.learner == "adam":
            st.m[k] = st.m[k] + (gk - st.m[k]) * (one - st.b1)
            st.v[k] = st.v[k] + (gk * gk - st.v[k]) * (one - st.b2)
            st.T[k] = st.T[k] - (st.m[k] * lr_t) / (np.sqrt(st.v[k]) + st.eps)
        else:
            st.T[k] = st.T[k] - st.lr * gk
    st.b1p, st.b2p = t(st.b1p * st.b1), t(st.b2p * st.b2)
    st.steps += 1
    return hinge, regl


def score(T, R, users, f, g):
    """D [n, I] of `users` against every item, as evaluate() computes it from the whole matrix"""
    users = np.asarray(users, np.int64)
    _, _, _, Yu, Yi = forward(T, R, users, np.arange(R.shape[1]), f, g)
    return (Yu + Yi) * T["UV"].dtype.type(0.5)


# ---------------------------------------------------------------------------------------------- the draw rule
def draw_negatives(seed, epoch, i, j, a, bp, observed, n_cols, num_neg):
    """the num_neg negatives of the positive at block cell (a, bp): `observed` the set of the row's observed block
    columns.  A pure function of its arguments."""
    key = (seed ^ splitmix64(((i & 0xFFFFFFFF) << 32) | (j & 0xFFFFFFFF))) & M64
    taken = []
    for k in range(num_neg):
        gen = XorShift64s(key, epoch & M64, (a * 512 + bp) * 8 + k)
        neg = -1
        for _ in range(MAX_REJECTS):
            cand = (gen.next() * n_cols) >> 64
            if cand not in observed and cand not in taken:
                neg = cand
                break
        if neg < 0:
            rank = (gen.next() * (n_cols - len(observed) - k)) >> 64
            free = [x for x in range(n_cols) if x not in observed and x not in taken]
            neg = free[rank]
        taken.append(int(neg))
    return taken


def block_bits(indptr, indices, rows, cols):
    """per block row the ascending list of its observed block columns"""
    pos = {int(c): b for b, c in enumerate(cols)}
    out = []
    for u in rows:
        row = indices[indptr[u]:indptr[u + 1]]
        out.append(sorted(pos[int(x)] for x in row if int(x) in pos))
    return out


def draw_pairs(indptr, indices, rows, cols, seed, epoch, i, j, num_neg):
    """(a, bp, bn) int64 arrays: row-major over the block's stored entries, num_neg pairs each; a block row with fewer
    than num_neg unobserved columns gives none"""
    A, P, N = [], [], []
    n_cols = len(cols)
    for a, obs in enumerate(block_bits(indptr, indices, rows, cols)):
        if not obs or n_cols - len(obs) < num_neg:
            continue
        have = set(obs)
        for bp in obs:
            for bn in draw_negatives(seed, epoch, i, j, a, bp, have, n_cols, num_neg):
                A.append(a)
                P.append(bp)
                N.append(bn)
    return np.asarray(A, np.int64), np.asarray(P, np.int64), np.asarray(N, np.int64)


def golden_tables(g, case, init, s):
    """{name: float64 table} after step s of the golden's float64 run, and {name: the float32 run's distance}"""
    want = {k: init[k].astype(np.float64) + g["%s_f64_%s" % (case, k)][s] for k in NAMES}
    gap = {k: float(g["%s_gap_%s" % (case, k)][s]) for k in NAMES}
    return want, gap
