"""A numpy restatement of ConvNCF (model/general_recommender/ConvNCF.py:87-145, util/learner.py's pairwise losses,
TF-1.12's Adagrad kernels) for the ConvNCF tests, with hand-written gradients: the forward pass, the loss, every gradient,
one training step (sparse Adagrad at lr_embed for the two tables, dense Adagrad at lr_net for everything else, both
accumulators starting at 0.1) and the scores of all items.  Every function takes `dtype`: float64 is the yardstick,
float32 the same arithmetic in single precision, whose distance from the float64 form is the allowance of the GPU tests
on the shapes no golden holds.  Tied to torch autograd (F.conv2d, stride 2) and to the reference class's own trace in
test_convncf_cpu.py.

Variables, by name: embedding_P [U, d], embedding_Q [I, d]; per layer k = 0..L-1 kernel<k> [2, 2, c_in, c_out] and bias<k>
[c_out] (c_in = 1 for the first); W [c_last, 1], b [1].  d == 2^L: the last layer has one position.

With a 2x2 kernel, stride 2 and even sizes SAME pads nothing: layer k is a product of the non-overlapping 2x2 patches
[positions, 4 c_in] (corner (i, j) major, channel minor — the row order of kernel.reshape(4 c_in, c_out)) with the kernel."""
import numpy as np

LR_EMBED, LR_NET = 0.05, 0.1
ACC0 = 0.1                     # tf.train.AdagradOptimizer's initial_accumulator_value
# case -> (d, net_channel, loss, regs, lr_embed, lr_net, steps)
CASES = {
    "single": (2, [3], "bpr", [0.0, 0.0, 0.0], LR_EMBED, LR_EMBED, 3),
    "regs": (4, [3, 5], "bpr", [0.01, 0.02, 0.03], 0.03, 0.07, 3),
    "hinge": (8, [4, 8, 6], "hinge", [0.0, 0.0, 0.0], LR_EMBED, LR_NET, 3),
    "square": (16, [4, 8, 8, 6], "square", [0.0, 0.0, 0.0], LR_EMBED, LR_NET, 3),
    "default": (64, [32] * 6, "bpr", [0.01, 0.0, 0.0], LR_EMBED, LR_NET, 3),
}
PREDICT_CASES = ("regs", "square")
EPOCH_CASE = "hinge"
TABLES = ("embedding_P", "embedding_Q")


def names(n_layers):
    out = list(TABLES)
    for k in range(n_layers):
        out += ["kernel%d" % k, "bias%d" % k]
    return out + ["W", "b"]


def shapes(U, I, d, channels):
    out = {"embedding_P": (U, d), "embedding_Q": (I, d)}
    c_in = 1
    for k, c in enumerate(channels):
        out["kernel%d" % k], out["bias%d" % k] = (2, 2, c_in, int(c)), (int(c),)
        c_in = int(c)
    out["W"], out["b"] = (c_in, 1), (1,)
    return out


def init_tables(U, I, d, channels, seed, scale=1.0):
    """seeded float32 initial values: embeddings N(0, 0.5), kernels glorot-like uniform, biases U(-0.1, 0.3), W, b
    N(0, 0.5) — large enough that tanh is neither linear nor saturated"""
    rs = np.random.RandomState(seed)
    out = {}
    for n, shape in shapes(U, I, d, channels).items():
        if n.startswith("kernel"):
            lim = scale * np.sqrt(6.0 / (4 * shape[2] + shape[3]))
            out[n] = rs.uniform(-lim, lim, shape).astype(np.float32)
        elif n.startswith("bias"):
            out[n] = rs.uniform(-0.1, 0.3, shape).astype(np.float32)
        else:
            out[n] = (0.5 * rs.standard_normal(shape)).astype(np.float32)
    return out


def _cast(tab, dtype):
    return {k: np.asarray(v, dtype=dtype) for k, v in tab.items()}


def n_layers_of(tab):
    return sum(1 for k in tab if k.startswith("kernel"))


def patches(x):
    """[n, s, s, c] -> [n, s/2, s/2, 4 c]: entry (i, j, ch) of the 2x2 patch at (a, b) is x[2a + i, 2b + j, ch]"""
    n, s, _, c = x.shape
    return x.reshape(n, s // 2, 2, s // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, s // 2, s // 2, 4 * c)


def unpatches(dx):
    """the inverse of patches: [n, m, m, 4 c] -> [n, 2m, 2m, c]"""
    n, m, _, c4 = dx.shape
    c = c4 // 4
    return dx.reshape(n, m, m, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, 2 * m, 2 * m, c)


def forward(tab, users, items, dtype=np.float64):
    """(output [n], the layers' inputs as patches, the activations) — E = p (x) q rounded once, as the graph forms it"""
    tab = _cast(tab, dtype)
    users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
    p, q = tab["embedding_P"][users], tab["embedding_Q"][items]
    x = (p[:, :, None] * q[:, None, :])[..., None]
    xs, acts = [], []
    for k in range(n_layers_of(tab)):
        K = tab["kernel%d" % k]
        xp = patches(x)
        x = np.tanh(xp @ K.reshape(-1, K.shape[3]) + tab["bias%d" % k])
        xs.append(xp)
        acts.append(x)
    n, s = x.shape[0], x.shape[1]
    if s != 1:
        raise ValueError("embedding_size is not 2^len(net_channel)")
    out = x.reshape(n, -1) @ tab["W"][:, 0] + tab["b"][0]
    return out, xs, acts


def loss_and_dy(y, loss, dtype=np.float64):
    """learner.pairwise_loss, summed, and its derivative: bpr -sum log sigmoid(y), hinge sum max(y + 1, 0) as the
    reference's learner states it, square sum (1 - y)^2"""
    one = dtype(1.0)
    if loss == "bpr":
        term = np.maximum(-y, 0) + np.log1p(np.exp(-np.abs(y)))
        return term.sum(dtype=dtype), (-one / (one + np.exp(y))).astype(dtype)
    if loss == "hinge":
        return np.maximum(y + one, 0).sum(dtype=dtype), (y + one > 0).astype(dtype)
    if loss == "square":
        return ((one - y) ** 2).sum(dtype=dtype), (-2 * (one - y)).astype(dtype)
    raise Exception("please choose a suitable loss function")


def backward(tab, users, items, dout, xs, acts, dtype=np.float64):
    """the gradients of sum(dout * output) by hand: {dense name: gradient}, dp [n, d], dq [n, d]"""
    tab = _cast(tab, dtype)
    users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
    L = n_layers_of(tab)
    n = len(users)
    G = {}
    top = acts[-1].reshape(n, -1)
    G["W"] = (top * dout[:, None]).sum(axis=0)[:, None]
    G["b"] = np.asarray([dout.sum()], dtype=dtype)
    da = (dout[:, None] * tab["W"][:, 0][None, :]).reshape(acts[-1].shape)
    for k in range(L - 1, -1, -1):
        K = tab["kernel%d" % k]
        a = acts[k]
        dz = da * (1 - a * a)                              # tanh' = 1 - y^2; exactly 0 where tanh saturated to +-1
        G["kernel%d" % k] = (xs[k].reshape(-1, xs[k].shape[3]).T @ dz.reshape(-1, dz.shape[3])).reshape(K.shape)
        G["bias%d" % k] = dz.sum(axis=2).sum(axis=1).sum(axis=0)     # columns, rows, pairs: short float32 sums
        da = unpatches(dz @ K.reshape(-1, K.shape[3]).T)
    dE = da[..., 0]
    p, q = tab["embedding_P"][users], tab["embedding_Q"][items]
    dp = np.einsum("nrs,ns->nr", dE, q)
    dq = np.einsum("nrs,nr->ns", dE, p)
    return G, dp, dq


def gradients(tab, users, pos, neg, loss="bpr", regs=(0.0, 0.0, 0.0), dtype=np.float64):
    """((self.loss, the regs[0] term), {name: gradient of opt_loss}): the tables' gradients are the sums over the batch's
    occurrences of a row; the embedding regulariser is on the gathered rows p1, q2, q1 — never p2"""
    tab = _cast(tab, dtype)
    users, pos, neg = (np.asarray(v, np.int64) for v in (users, pos, neg))
    L = n_layers_of(tab)
    r0, r1, r2 = (dtype(r) for r in regs)
    yp, xs_p, acts_p = forward(tab, users, pos, dtype)
    yn, xs_n, acts_n = forward(tab, users, neg, dtype)
    term, dy = loss_and_dy(yp - yn, loss, dtype)
    Gp, dp1, dq1 = backward(tab, users, pos, dy, xs_p, acts_p, dtype)
    Gn, dp2, dq2 = backward(tab, users, neg, -dy, xs_n, acts_n, dtype)
    G = {k: Gp[k] + Gn[k] for k in Gp}
    for k in range(L):
        for n in ("kernel%d" % k, "bias%d" % k):
            G[n] = G[n] + r2 * tab[n]
    for n in ("W", "b"):
        G[n] = G[n] + r1 * tab[n] + r2 * tab[n]
    p, q1, q2 = tab["embedding_P"][users], tab["embedding_Q"][pos], tab["embedding_Q"][neg]
    G["embedding_P"] = np.zeros_like(tab["embedding_P"])
    G["embedding_Q"] = np.zeros_like(tab["embedding_Q"])
    np.add.at(G["embedding_P"], users, dp1 + r0 * p)
    np.add.at(G["embedding_P"], users, dp2)
    np.add.at(G["embedding_Q"], pos, dq1 + r0 * q1)
    np.add.at(G["embedding_Q"], neg, dq2 + r0 * q2)
    reg = r0 * dtype(0.5) * ((p * p).sum() + (q1 * q1).sum() + (q2 * q2).sum())
    return (float(term), float(reg)), {n: G[n] for n in names(L)}


def opt_loss(tab, users, pos, neg, loss, regs):
    """the scalar the optimisers minimise, in float64"""
    tab = _cast(tab, np.float64)
    users, pos, neg = (np.asarray(v, np.int64) for v in (users, pos, neg))
    L = n_layers_of(tab)
    y = forward(tab, users, pos)[0] - forward(tab, users, neg)[0]
    l2 = lambda *vs: sum(0.5 * (v * v).sum() for v in vs)
    head = l2(tab["W"], tab["b"])
    net = sum(l2(tab["kernel%d" % k], tab["bias%d" % k]) for k in range(L))
    return float(loss_and_dy(y, loss)[0] + regs[0] * l2(tab["embedding_P"][users], tab["embedding_Q"][neg],
                                                        tab["embedding_Q"][pos]) + regs[1] * head + regs[2] * (net + head))


def scores(tab, users, dtype=np.float64):
    """[n, I]: predict() in full mode — every item for each user"""
    I = len(tab["embedding_Q"])
    users = np.asarray(users, np.int64)
    return np.stack([forward(tab, np.full(I, u), np.arange(I), dtype)[0] for u in users]) if len(users) else \
        np.zeros((0, I), dtype)


class State:
    """the variables and their Adagrad accumulators; step() is one sess.run((self.loss, self.optimizer))"""

    def __init__(self, tab, loss="bpr", regs=(0.0, 0.0, 0.0), lr_embed=LR_EMBED, lr_net=LR_NET, dtype=np.float64,
                 acc0=ACC0):
        self.dtype = dtype
        self.var = {k: np.array(v, dtype=dtype) for k, v in tab.items()}
        self.acc = {k: np.full_like(v, acc0) for k, v in self.var.items()}
        self.loss, self.regs, self.lr_embed, self.lr_net = loss, tuple(regs), dtype(lr_embed), dtype(lr_net)

    def step(self, users, pos, neg):
        """returns the pre-update (self.loss, the regs[0] term)"""
        loss2, G = gradients(self.var, users, pos, neg, self.loss, self.regs, self.dtype)
        for key, g in G.items():
            var, acc = self.var[key], self.acc[key]
            if key == "embedding_P":                       # the sparse form: the touched rows only, duplicates summed
                r, lr = np.unique(np.asarray(users, np.int64)), self.lr_embed
            elif key == "embedding_Q":
                r, lr = np.unique(np.concatenate([np.asarray(pos, np.int64), np.asarray(neg, np.int64)])), self.lr_embed
            else:
                r, lr = slice(None), self.lr_net
            acc[r] += g[r] * g[r]
            var[r] -= (lr * g[r]) / np.sqrt(acc[r])
        return loss2
