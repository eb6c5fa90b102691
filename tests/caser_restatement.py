"""A numpy restatement of the Caser graph (model/sequential_recommender/Caser.py:70-122 of the reference): forward, loss,
every gradient by hand, both forms of TF-1.12's Adam.  float64 by default; `dtype=np.float32` evaluates the same
expressions in float32, which is what the saturation test needs of the loss tail (`loss_tail`).

Notation: I items, d factors_num, L seq_L, T seq_T, N neg_samples, F = nv d + nh L.  Variables in creation order
(`table_names`): user_embeddings [U, d], seq_item_embeddings [I, d], item_embeddings [I, 2d], item_biases [I],
conv_v_kernel [L, nv], conv_v_bias [nv], conv_h<i>_kernel [i, d, nh] and conv_h<i>_bias [nh] for i = 1..L, fc1_kernel
[F, d], fc1_bias [d].

`ties`: how reduce_max's gradient treats tied positions — "even" is TF's (equal shares), "first" the device kernel's
(the first maximum takes all).  tests/test_caser_cpu.py asserts they agree where windows tie by holding equal inputs.

A pad id (I, or anything outside [0, I)) in seq reads the zero row; among the targets it reads a zero row and a zero
bias (TF on a GPU), so its logit is 0, it has no gradient and it stays in the mean.
"""
import numpy as np

from sasrec_restatement import numpy_batch_randint_choice                  # noqa: F401  (the traces' sampler stand-in)

LR = 0.001
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
LOG_EPS = 1e-24
# case -> (factors_num, seq_L, seq_T, neg_samples, nv, nh, l2_reg, dropout)
CASES = {"first": (8, 5, 3, 3, 4, 4, 0.001, 0.0), "second": (50, 5, 3, 3, 4, 16, 0.001, 0.5),
         "third": (3, 1, 1, 1, 1, 1, 0.0, 0.0), "fourth": (12, 7, 2, 5, 3, 5, 0.0, 0.3)}
PREDICT_CASE = "second"
TABLES = ("user_embeddings", "seq_item_embeddings", "item_embeddings", "item_biases")
SPARSE_FORM = ("user_embeddings", "item_embeddings", "item_biases")       # at l2_reg == 0


def table_names(seq_L):
    out = list(TABLES) + ["conv_v_kernel", "conv_v_bias"]
    for i in range(1, seq_L + 1):
        out += ["conv_h%d_kernel" % i, "conv_h%d_bias" % i]
    return out + ["fc1_kernel", "fc1_bias"]


def init_tables(n_users, n_items, d, L, nv, nh, seed):
    """small random values for every variable, the biases included (a zero bias hides the pad windows); sized so that
    features, z and the logits are O(1) and no sigmoid saturates"""
    rs = np.random.RandomState(seed)
    F = nv * d + nh * L
    t = {"user_embeddings": rs.randn(n_users, d) * 0.4, "seq_item_embeddings": rs.randn(n_items, d) * 0.5,
         "item_embeddings": rs.randn(n_items, 2 * d) * (0.8 / np.sqrt(2 * d)), "item_biases": rs.randn(n_items) * 0.1,
         "conv_v_kernel": rs.randn(L, nv) * (0.8 / np.sqrt(L)), "conv_v_bias": rs.randn(nv) * 0.1}
    for i in range(1, L + 1):
        t["conv_h%d_kernel" % i] = rs.randn(i, d, nh) * (1.0 / np.sqrt(i * d))
        t["conv_h%d_bias" % i] = rs.randn(nh) * 0.1
    t["fc1_kernel"], t["fc1_bias"] = rs.randn(F, d) * (1.5 / np.sqrt(F)), rs.randn(d) * 0.1
    return {k: v.astype(np.float32) for k, v in t.items()}


def _padded(table, dt):
    return np.concatenate([np.asarray(table, dt), np.zeros((1,) + np.shape(table)[1:], dt)], axis=0)


def _clip(ids, n):
    ids = np.asarray(ids, np.int64)
    return np.where((ids < 0) | (ids >= n), n, ids)


def loss_tail(pos_logit, neg_logit, dtype=np.float64):
    """the loss of Caser.py:109-111 as it is written, and d loss / d logit with TF's SigmoidGrad y (1 - y), in `dtype`:
    (loss, d_pos, d_neg).  In float32 a logit beyond about 17 has sigmoid exactly 1: a negative there costs exactly
    -log(1e-24) and has gradient 0"""
    dt = dtype
    one, eps = dt(1.0), dt(LOG_EPS)
    with np.errstate(over="ignore"):
        yp = one / (one + np.exp(-np.asarray(pos_logit, dt)))
        yn = one / (one + np.exp(-np.asarray(neg_logit, dt)))
    ap, an = yp + eps, (one - yn) + eps
    loss = np.mean(-np.log(ap), dtype=dt) + np.mean(-np.log(an), dtype=dt)
    d_pos = -(yp * (one - yp)) / ap / dt(yp.size)
    d_neg = (yn * (one - yn)) / an / dt(yn.size)
    return dt(loss), d_pos.astype(dt), d_neg.astype(dt)


def forward(T, users, seq, n_items, nv, nh, rate=0.0, mask=None, training=False, ties="even", dtype=np.float64):
    """everything up to p = concat(z, user row) [B, 2d], and what the backward pass needs"""
    dt = dtype
    seq = _clip(seq, n_items)
    B, L = seq.shape
    d = np.shape(T["user_embeddings"])[1]
    E = _padded(T["seq_item_embeddings"], dt)[seq]                                       # [B, L, d]
    Kv, bv = np.asarray(T["conv_v_kernel"], dt), np.asarray(T["conv_v_bias"], dt)
    out_v = (np.einsum("btj,tc->bjc", E, Kv) + bv).reshape(B, d * nv)                    # feature j nv + c
    feats, saved = [out_v], []
    for i in range(1, L + 1):
        K, bh = np.asarray(T["conv_h%d_kernel" % i], dt), np.asarray(T["conv_h%d_bias" % i], dt)
        win = np.stack([E[:, p:p + i, :] for p in range(L - i + 1)], axis=1)             # [B, P, i, d]
        act = np.maximum(np.einsum("bptj,tjc->bpc", win, K) + bh, dt(0))                 # relu, then the max
        pooled = act.max(axis=1)
        if ties == "even":
            hit = (act == pooled[:, None, :]).astype(dt)
            share = hit / hit.sum(axis=1, keepdims=True)
        else:
            share = np.zeros_like(act)
            first = act.argmax(axis=1)                                                   # the first maximum
            np.put_along_axis(share, first[:, None, :], dt(1), axis=1)
        feats.append(pooled)
        saved.append((win, act, share))
    feat = np.concatenate(feats, axis=1)
    if training and rate:
        fac = np.asarray(mask, dt) / dt(1.0 - rate)                                      # x / keep_prob * mask
    else:
        fac = np.ones_like(feat)
    x = feat * fac
    pre = x @ np.asarray(T["fc1_kernel"], dt) + np.asarray(T["fc1_bias"], dt)
    z = np.maximum(pre, dt(0))
    users = np.asarray(users, np.int64)
    p = np.concatenate([z, np.asarray(T["user_embeddings"], dt)[users]], axis=1)
    return p, dict(E=E, seq=seq, saved=saved, fac=fac, x=x, pre=pre, users=users)


def gradients(T, users, seq, pos, neg, n_items, nv, nh, rate=0.0, l2_reg=0.0, mask=None, ties="even", dtype=np.float64):
    """(loss + regulariser, {name: gradient}) of one step"""
    dt = dtype
    I = n_items
    p, s = forward(T, users, seq, I, nv, nh, rate, mask, True, ties, dt)
    B, L = s["seq"].shape
    d = p.shape[1] // 2
    n_pos = np.shape(pos)[1]
    tar = _clip(np.concatenate([pos, neg], axis=1), I)                                   # [B, T + N]
    real = tar != I
    Q, qb = _padded(T["item_embeddings"], dt), _padded(T["item_biases"], dt)
    logit = np.einsum("bc,bkc->bk", p, Q[tar]) + qb[tar]
    loss, d_pos, d_neg = loss_tail(logit[:, :n_pos], logit[:, n_pos:], dt)
    g = np.concatenate([d_pos, d_neg], axis=1) * real
    G = {k: np.zeros(np.shape(v), dt) for k, v in T.items()}
    b_of = np.broadcast_to(np.arange(B)[:, None], tar.shape)
    np.add.at(G["item_embeddings"], tar[real], g[real][:, None] * p[b_of[real]])
    np.add.at(G["item_biases"], tar[real], g[real])
    dp = np.einsum("bk,bkc->bc", g, Q[tar])
    np.add.at(G["user_embeddings"], s["users"], dp[:, d:])
    dz = dp[:, :d] * (s["pre"] > 0)
    Wfc = np.asarray(T["fc1_kernel"], dt)
    G["fc1_kernel"], G["fc1_bias"] = s["x"].T @ dz, dz.sum(axis=0)
    dfeat = (dz @ Wfc.T) * s["fac"]
    E = s["E"]
    dv = dfeat[:, :nv * d].reshape(B, d, nv)
    G["conv_v_kernel"], G["conv_v_bias"] = np.einsum("btj,bjc->tc", E, dv), dv.sum(axis=(0, 1))
    dE = np.einsum("bjc,tc->btj", dv, np.asarray(T["conv_v_kernel"], dt))
    for i in range(1, L + 1):
        win, act, share = s["saved"][i - 1]
        dh = dfeat[:, nv * d + (i - 1) * nh:nv * d + i * nh]
        dconv = dh[:, None, :] * share * (act > 0)
        G["conv_h%d_kernel" % i] = np.einsum("bpc,bptj->tjc", dconv, win)
        G["conv_h%d_bias" % i] = dconv.sum(axis=(0, 1))
        dwin = np.einsum("bpc,tjc->bptj", dconv, np.asarray(T["conv_h%d_kernel" % i], dt))
        for q in range(L - i + 1):
            dE[:, q:q + i, :] += dwin[:, q]
    at = s["seq"] != I                                                                   # the pad row takes no gradient
    np.add.at(G["seq_item_embeddings"], s["seq"][at], dE[at])
    if l2_reg:
        for k in TABLES:                                                                 # the get_variable tables only
            v = np.asarray(T[k], dt)
            loss = loss + dt(l2_reg) * np.sum(v * v, dtype=dt) / dt(2)
            G[k] += dt(l2_reg) * v
    return dt(loss), G


def scores(T, users, seq, n_items, nv, nh, dtype=np.float64):
    """predict(): concat(z, user row) . item_embeddings^T, without the item biases (Caser.py:122)"""
    p, _ = forward(T, users, seq, n_items, nv, nh, dtype=dtype)
    return p @ np.asarray(T["item_embeddings"], dtype).T


class Adam:
    """TF-1.12's Adam as the optimiser picks its forms for this graph: without a regulariser the three tables that are
    gathered from the variable take the sparse form (which still sweeps every row); seq_item_embeddings, read through a
    concat, and everything else take ApplyAdam; with a regulariser every variable does"""

    def __init__(self, tables, l2_reg, dtype=np.float64, lr=LR, sparse=None):
        self.dt = dtype
        self.m = {k: np.zeros(np.shape(v), dtype) for k, v in tables.items()}
        self.v = {k: np.zeros(np.shape(v), dtype) for k, v in tables.items()}
        self.lr, self.b1, self.b2, self.eps = dtype(lr), dtype(BETA1), dtype(BETA2), dtype(EPS)
        self.b1p, self.b2p = self.b1, self.b2
        self.sparse = set(sparse) if sparse is not None else (set(SPARSE_FORM) if not l2_reg else set())

    def apply(self, T, G):
        one = self.dt(1.0)
        alpha = self.lr * np.sqrt(one - self.b2p) / (one - self.b1p)
        for k in T:
            m, v, g = self.m[k], self.v[k], G[k]
            if k in self.sparse:
                m[...] = m * self.b1 + g * (one - self.b1)
                v[...] = v * self.b2 + (g * g) * (one - self.b2)
                T[k] = T[k] - alpha * m / (np.sqrt(v) + self.eps)
            else:
                m += (g - m) * (one - self.b1)
                v += (g * g - v) * (one - self.b2)
                T[k] = T[k] - (m * alpha) / (np.sqrt(v) + self.eps)
        self.b1p, self.b2p = self.b1p * self.b1, self.b2p * self.b2


def train(tables, feeds, n_items, nv, nh, rate, l2_reg, masks=None, ties="even", dtype=np.float64, lr=LR, sparse=None):
    """the tables after each step of `feeds` [(users, seq, pos, neg)], and the losses before each update"""
    T = {k: np.asarray(v, dtype) for k, v in tables.items()}
    opt = Adam(T, l2_reg, dtype, lr, sparse)
    out, losses = [], []
    for s, (users, seq, pos, neg) in enumerate(feeds):
        loss, G = gradients(T, users, seq, pos, neg, n_items, nv, nh, rate, l2_reg,
                            None if masks is None else masks[s], ties, dtype)
        opt.apply(T, G)
        out.append({k: v.copy() for k, v in T.items()})
        losses.append(loss)
    return out, losses
