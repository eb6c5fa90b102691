"""A restatement of DeepICF (DeepICF.py:112-178, util/learner.py, TF-1.12's optimiser kernels and contrib batch_norm)
for the DeepICF tests: one training step in float64 numpy with HAND-WRITTEN gradients on the padded form, and predict().
It is independent of the derivation in csrc/deepicf.hip, is compared with the reference class's own float64 trace in
test_deepicf_cpu.py (and once with torch autograd), and serves the GPU tests for the shapes the trace does not hold.

The model: NAIS's attention pooling p (nais_restatement has the autograd form), then
    x0 = (num_idx^alpha p) (.) q;  per layer  z = x W_i + b_i,  [batch norm],  relu;  out = x_L w_out + b_out
    output = sigmoid(out + bias[item]);  loss = MEAN(-y log(output + 1e-7) - (1 - y) log(1 - output + 1e-7)) + regs
Batch norm is tf.contrib.layers.batch_norm(decay=0.9, epsilon=0.001) on a rank-2 input, which TF-1.12 sends down the
fused path: training normalises with the batch mean and the BIASED batch variance; the moving mean / variance move by
v -= (v - batch) * (1 - 0.9), the variance entering with Bessel's correction N / max(N - 1, 1) (`bessel=False` drops
it); predict() normalises with the moving statistics and moves nothing.

Optimiser forms: `bias` alone is read only through embedding_lookup (the sparse application, on the batch's items);
every other variable is dense — embedding_Q and c1 because the loss regularises the whole tables.  With batch norm on,
the gradient of a pre-norm bias b_i is zero in exact arithmetic; the restatement (and the device) write exact zeros.
"""
import numpy as np

import fism_restatement as F

BN_EPS, BN_DECAY, LOG_EPS = 0.001, 0.9, 1e-7


def names(n_layers, batch_norm):
    """the trainable variables in the order the class creates them, then the batch-norm pairs"""
    out = ["c1", "Q", "bias", "W", "b", "h", "Wout", "bout"]
    for i in range(n_layers):
        out += ["W%d" % i, "b%d" % i]
    if batch_norm:
        for i in range(n_layers):
            out += ["beta%d" % i, "gamma%d" % i]
    return out


def moving_names(n_layers, batch_norm):
    return ["mm%d" % i for i in range(n_layers)] + ["mv%d" % i for i in range(n_layers)] if batch_norm else []


def init_tables(I, d, w, layers, algorithm, batch_norm, seed, bias_scale=1.0):
    """float32 initial values, large enough that every term of the model matters at the toy sizes; bias_scale: a
    factor on `bias` (large: outputs near 0 and 1, where the 1e-7 inside the loss's logarithms matters)"""
    rs = np.random.RandomState(seed)
    f = lambda x: x.astype(np.float32)
    sign = np.where(rs.rand(w) < 0.5, -1.0, 1.0)
    T = dict(c1=f(0.3 * rs.randn(I, d)), Q=f(0.3 * rs.randn(I, d)), bias=f(bias_scale * 0.05 * rs.randn(I)),
             W=f(0.3 * rs.randn((algorithm + 1) * d, w)), b=f(sign * (0.3 + 0.2 * rs.rand(w))),
             h=f(1.0 + 0.3 * rs.randn(w)), Wout=f(0.5 * rs.randn(layers[-1], 1)), bout=f(0.3 * rs.randn(1)))
    n0 = d
    for i, n1 in enumerate(layers):
        T["W%d" % i] = f(rs.randn(n0, n1) * (1.5 / np.sqrt(n0)))
        T["b%d" % i] = f(0.3 * rs.randn(n1))
        n0 = n1
    if batch_norm:
        for i, n1 in enumerate(layers):
            T["beta%d" % i] = f(0.2 * rs.randn(n1))
            T["gamma%d" % i] = f(1.0 + 0.2 * rs.randn(n1))
            T["mm%d" % i] = np.zeros(n1, np.float32)
            T["mv%d" % i] = np.ones(n1, np.float32)
    return T


class State(F.State):
    """the variables (trainable and moving) and the slots of one learner"""

    def __init__(self, tables, hyper, learner="adam", lr=0.001, momentum=0.9):
        self.hyper = hyper
        L, bn = len(hyper["layers"]), bool(hyper["batch_norm"])
        self.names, self.moving = names(L, bn), moving_names(L, bn)
        self.var = {k: np.array(tables[k], dtype=np.float64) for k in self.names + self.moving}
        self.learner, self.lr, self.momentum = learner, lr, momentum
        init = {"adam": 0.0, "gd": 0.0, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        self.s0 = {k: np.full_like(self.var[k], init) for k in self.names}
        self.s1 = {k: np.zeros_like(self.var[k]) for k in self.names}
        self.b1p, self.b2p = 0.9, 0.999


def _act(z, activation):
    if activation == 0:
        return np.maximum(z, 0.0)
    if activation == 1:
        return 1.0 / (1.0 + np.exp(-z))
    if activation == 2:
        return np.tanh(z)
    return z


def _dact(z, a, activation):
    if activation == 0:
        return (z > 0).astype(z.dtype)
    if activation == 1:
        return a * (1.0 - a)
    if activation == 2:
        return 1.0 - a * a
    return np.ones_like(z)


def padded(R, inst, mask):
    """(ids [B, L] padded with num_items, mask [B, L], items [B], num_idx [B]) of the instances: the mask is
    sequence_mask(num_idx) cut at the longest history ("reference": one zero row inside it for every shorter
    instance), or the history alone ("history")"""
    I = R.shape[1]
    hist = [F.history(R, u, e) for u, _, e, _, _ in inst]
    L = max([len(x) for x in hist], default=0)
    ids = np.full((len(inst), L), I, np.int64)
    m = np.zeros((len(inst), L))
    for k, x in enumerate(hist):
        ids[k, :len(x)] = x
        m[k, :min(L, len(x) + (1 if mask == "reference" else 0))] = 1.0
    return ids, m, np.asarray([i for _, i, _, _, _ in inst], np.int64), np.asarray([float(x[3]) for x in inst])


def attention(V, hy, ids, m, item, n):
    """the pooled, scaled vector pc [B, d] and what the backward pass needs"""
    alg, act = hy["algorithm"], hy["activation"]
    c1, Q = V["c1"], V["Q"]
    table = np.concatenate([c1, np.zeros((1, c1.shape[1]))], axis=0)
    c = table[ids]                                              # [B, L, d]
    q = Q[item]                                                 # [B, d]
    qq = np.broadcast_to(q[:, None, :], c.shape)
    x = c * qq if alg == 0 else np.concatenate([c, qq], axis=2)
    z = x @ V["W"] + V["b"][None, None, :]
    a = _act(z, act)
    e = np.exp(a @ V["h"]) * m
    S = e.sum(axis=1)
    S = np.where(S > 0, S, 1.0)                                # an empty mask: p = 0
    A = e / (S ** hy["beta"])[:, None]
    p = (A[:, :, None] * c).sum(axis=1)
    coeff = n ** hy["alpha"]                                   # the exponent is +alpha (DeepICF.py:155)
    return dict(c=c, q=q, x=x, z=z, a=a, e=e, S=S, A=A, p=p, coeff=coeff, pc=coeff[:, None] * p)


def tower(V, hy, x0, training, bessel=True, moving_in_training=False):
    """(out [B], per-layer caches, the new moving statistics {name: value} of a training pass)"""
    x, caches, moved = x0, [], {}
    for i in range(len(hy["layers"])):
        z = x @ V["W%d" % i] + V["b%d" % i][None, :]
        cache = dict(x=x, z=z)
        if hy["batch_norm"]:
            if training and not moving_in_training:
                N = z.shape[0]
                mu = z.mean(axis=0)
                var = ((z - mu[None, :]) ** 2).mean(axis=0)
                unbiased = var * (N / max(N - 1, 1)) if bessel else var
                moved["mm%d" % i] = V["mm%d" % i] - (V["mm%d" % i] - mu) * (1 - BN_DECAY)
                moved["mv%d" % i] = V["mv%d" % i] - (V["mv%d" % i] - unbiased) * (1 - BN_DECAY)
            else:
                mu, var = V["mm%d" % i], V["mv%d" % i]
            rstd = 1.0 / np.sqrt(var + BN_EPS)
            xhat = (z - mu[None, :]) * rstd[None, :]
            y = V["gamma%d" % i][None, :] * xhat + V["beta%d" % i][None, :]
            cache.update(rstd=rstd, xhat=xhat)
        else:
            y = z
        cache["y"] = y
        caches.append(cache)
        x = np.maximum(y, 0.0)
    out = (x @ V["Wout"] + V["bout"][None, :]).sum(axis=1)
    return out, caches, x, moved


def _regw(hy):
    return {i: hy["regw"][i] for i in range(min(len(hy["layers"]), len(hy["regw"]))) if hy["regw"][i] > 0}


def loss_and_gradients(V, R, users, items, labels, hy, mask="reference", bessel=True, variant=None):
    """(loss, {name: dense gradient}, new moving statistics).  variant: None, or the name of a deliberate mistake
    (tests/test_deepicf_cpu.py shows that each is told from the model by the golden trace)"""
    inst = F.instances(R, users, items, labels, False)
    ids, m, item, n = padded(R, inst, mask)
    y = np.asarray(labels, np.float64)
    B = len(y)
    hy2 = dict(hy, alpha=-hy["alpha"]) if variant == "neg_alpha" else hy
    at = attention(V, hy2, ids, m, item, n)
    q, c = at["q"], at["c"]
    x0 = at["pc"] * q
    out, caches, xL, moved = tower(V, hy, x0, True, bessel, moving_in_training=variant == "moving_in_training")
    logit = out + V["bias"][item]
    prob = 1.0 / (1.0 + np.exp(-logit))
    eps = 0.0 if variant == "no_eps" else LOG_EPS
    scale = 1.0 if variant == "sum_loss" else 1.0 / B
    loss = scale * (-y * np.log(prob + eps) - (1 - y) * np.log(1 - prob + eps)).sum()
    regs = hy["regs"]
    loss += regs[0] * 0.5 * (V["Q"] ** 2).sum() + regs[1] * 0.5 * (V["c1"] ** 2).sum() + \
        regs[2] * 0.5 * (V["W"] ** 2).sum()
    regw = _regw(hy)
    if variant == "regw_all" and hy["regw"]:
        regw = {i: hy["regw"][min(i, len(hy["regw"]) - 1)] for i in range(len(hy["layers"]))}
    for i, r in regw.items():
        loss += r * 0.5 * (V["W%d" % i] ** 2).sum()

    G = {k: np.zeros_like(V[k]) for k in names(len(hy["layers"]), hy["batch_norm"])}
    dlogit = scale * (-y / (prob + eps) + (1 - y) / (1 - prob + eps)) * prob * (1 - prob)
    np.add.at(G["bias"], item, dlogit)
    G["bout"][0] = dlogit.sum()
    G["Wout"][:, 0] = xL.T @ dlogit
    dx = dlogit[:, None] * V["Wout"][:, 0][None, :]
    for i in reversed(range(len(hy["layers"]))):
        cch = caches[i]
        dy = dx * (cch["y"] > 0)
        if hy["batch_norm"]:
            xhat, rstd = cch["xhat"], cch["rstd"]
            G["gamma%d" % i] = (dy * xhat).sum(axis=0)
            G["beta%d" % i] = dy.sum(axis=0)
            dxh = dy * V["gamma%d" % i][None, :]
            if variant == "moving_in_training":
                dz = dxh * rstd[None, :]
                G["b%d" % i] = dz.sum(axis=0)
            else:
                cross = 0.0 if variant == "no_xhat_term" else xhat * (dxh * xhat).mean(axis=0)[None, :]
                dz = (dxh - dxh.mean(axis=0)[None, :] - cross) * rstd[None, :]
                G["b%d" % i][:] = 0.0                           # exact: sum_b dz = 0
        else:
            dz = dy
            G["b%d" % i] = dz.sum(axis=0)
        G["W%d" % i] = cch["x"].T @ dz
        dx = dz @ V["W%d" % i].T
    for i, r in regw.items():
        G["W%d" % i] += r * V["W%d" % i]
    # x0 = pc (.) q
    dq = dx * at["pc"]
    g = (dx * q) * at["coeff"][:, None]                         # d loss / d p
    alg, act, d = hy["algorithm"], hy["activation"], q.shape[1]
    A, e, S = at["A"], at["e"], at["S"]
    dA_c = (c * g[:, None, :]).sum(axis=2)                      # g . c_j (0 on the padding row)
    gp = (g * at["p"]).sum(axis=1)
    ds = A * dA_c - hy["beta"] * (e / S[:, None]) * gp[:, None]
    dc = A[:, :, None] * g[:, None, :]
    G["h"] = (ds[:, :, None] * at["a"]).sum(axis=(0, 1))
    dz = ds[:, :, None] * V["h"][None, None, :] * _dact(at["z"], at["a"], act)
    G["b"] = dz.sum(axis=(0, 1))
    G["W"] = np.einsum("blk,blm->km", at["x"], dz)
    dxa = dz @ V["W"].T
    if alg == 0:
        dc = dc + dxa * q[:, None, :]
        dq = dq + (dxa * c).sum(axis=1)
    else:
        dc = dc + dxa[:, :, :d]
        dq = dq + dxa[:, :, d:].sum(axis=1)
    I = V["c1"].shape[0]
    gc = np.zeros((I + 1, d))
    np.add.at(gc, ids.reshape(-1), dc.reshape(-1, d))
    G["c1"] = gc[:I] + regs[1] * V["c1"]
    np.add.at(G["Q"], item, dq)
    G["Q"] += regs[0] * V["Q"]
    G["W"] += regs[2] * V["W"]
    return float(loss), G, moved, item


def step(st, R, users, items, labels, mask="reference", bessel=True, variant=None):
    """one sess.run((loss, optimizer)) with is_train_phase = True: the pre-update loss"""
    loss, G, moved, item = loss_and_gradients(st.var, R, users, items, labels, st.hyper, mask, bessel, variant)
    rows = np.unique(item)
    for k in st.names:
        if k == "bias" or (k == "Q" and variant == "q_rows"):
            st.apply(k, G[k], rows)
        else:
            st.apply(k, G[k], None)
    st.b1p, st.b2p = st.b1p * 0.9, st.b2p * 0.999
    for k, v in moved.items():
        st.var[k] = v
    return loss


def predict(R, V, hy, users):
    """DeepICF.py:246-258: the whole train row, the exact mask, num_idx = |R_u|, every item, the moving statistics; a
    user without train items scores through an empty pooling (p = 0)"""
    V = {k: np.asarray(v, np.float64) for k, v in V.items()}
    I = R.shape[1]
    out = np.empty((len(users), I))
    for k, u in enumerate(users):
        row = R.indices[R.indptr[u]:R.indptr[u + 1]].astype(np.int64)
        ids = np.tile(row, (I, 1))
        at = attention(V, hy, ids, np.ones(ids.shape), np.arange(I), np.full(I, float(len(row))))
        o, _, _, _ = tower(V, hy, at["pc"] * at["q"], False)
        out[k] = 1.0 / (1.0 + np.exp(-(o + V["bias"])))
    return out


# ------------------------------------------------------------------ the golden trace (tests/golden/make_golden_deepicf.py)
def load_trace(load_golden):
    """the two fixture files as one mapping"""
    g = dict(load_golden("tfgraph_deepicf"))
    g.update(load_golden("tfgraph_deepicf_more"))
    return g


def golden_matrix(g, case):
    import scipy.sparse as sp
    U, I = (int(x) for x in g["shape"])
    pre = "epoch_" if case == "epoch" else ""
    ind = g[pre + "indices"]
    return sp.csr_matrix((np.ones(len(ind), np.float32), ind, g[pre + "indptr"]), shape=(U, I))


def golden_hyper(g, case):
    import json
    return json.loads(str(g[case + "_hyper_json"]))


def golden_init(g, case):
    hy = golden_hyper(g, case)
    return init_tables(int(g["shape"][1]), hy["d"], hy["w"], hy["layers"], hy["algorithm"], hy["batch_norm"],
                       int(g[case + "_init_seed"]), hy.get("bias_scale", 1.0))


def golden_batches(g, case):
    """[(users, items, labels)] of the case's steps"""
    if case == "epoch":
        ends = np.cumsum(g["epoch_sizes"])
        return [(g["epoch_users"][e - n:e], g["epoch_items"][e - n:e], g["epoch_labels"][e - n:e])
                for e, n in zip(ends, g["epoch_sizes"])]
    return [tuple(g["%s_%s_%d" % (case, k, s)] for k in ("users", "items", "labels"))
            for s in range(int(g[case + "_steps"]))]


def golden_var(g, case, init, name, step):
    """the variable after `step` (0-based; the epoch holds its end alone) of the float64 run"""
    return init[name].astype(np.float64) + g["%s_f64_%s" % (case, name)][step]


def tolerance(g, case, name, step, want):
    """the project's standing tolerance: 4 x the reference's own float32-to-float64 gap + 1e-5 max |want|"""
    return 4.0 * float(g["%s_gap_%s" % (case, name)][step]) + 1e-5 * float(np.abs(want).max(initial=0))
