"""A float64 numpy restatement of NeuMF and MLP (model/general_recommender/NeuMF.py:69-100, MLP.py, util/learner.py,
TF-1.12's optimiser kernels) for the NeuMF tests: the forward pass, the loss, every gradient, one training step for every
learner (sparse application for the four tables, dense for kernels and biases), the scores of all items, and the split
of the first layer the device scorer uses.  Checked against the reference classes' own f64 trace in test_neumf_cpu.py;
the GPU tests use it for the shapes the trace does not hold.

Variables, by name: mf_embedding_user [U, d], mf_embedding_item [I, d] (absent for MLP, d = 0), mlp_embedding_user [U, e],
mlp_embedding_item [I, e], e = int(layers[0] / 2); kernel<k> [in_k, layers[k]], bias<k> [layers[k]]."""
import numpy as np

LR = 0.001
# case -> (model, layers, embedding_size (0: MLP), loss, learner, reg_mf, reg_mlp, steps)
CASES = {
    "default": ("NeuMF", [64, 32, 16], 16, "cross_entropy", "adam", 0.0, 0.0, 4),
    "odd": ("NeuMF", [7, 5, 3], 3, "square", "adam", 0.01, 0.02, 4),
    "one": ("NeuMF", [10], 5, "cross_entropy", "adam", 0.0, 0.0, 4),
    "wide": ("NeuMF", [128, 64], 64, "cross_entropy", "adam", 0.0, 0.0, 4),
    "gd": ("NeuMF", [7, 5, 3], 3, "square", "gd", 0.01, 0.02, 2),
    "adagrad": ("NeuMF", [7, 5, 3], 3, "square", "adagrad", 0.01, 0.02, 2),
    "rmsprop": ("NeuMF", [7, 5, 3], 3, "square", "rmsprop", 0.01, 0.02, 2),
    "momentum": ("NeuMF", [7, 5, 3], 3, "square", "momentum", 0.01, 0.02, 2),
    "mlp": ("MLP", [8, 4], 0, "cross_entropy", "adam", 0.0, 0.01, 4),
}
PREDICT_CASES = ("odd", "default")
EPOCH_CASE = "default"
TABLES = ("mf_embedding_user", "mf_embedding_item", "mlp_embedding_user", "mlp_embedding_item")


def layer_inputs(layers):
    return [2 * (int(layers[0]) // 2)] + [int(w) for w in layers[:-1]]


def names(layers, d):
    out = list(TABLES[:2] if d else ()) + list(TABLES[2:])
    for k in range(len(layers)):
        out += ["kernel%d" % k, "bias%d" % k]
    return out


def shapes(U, I, d, layers):
    e = int(layers[0]) // 2
    out = {"mf_embedding_user": (U, d), "mf_embedding_item": (I, d), "mlp_embedding_user": (U, e),
           "mlp_embedding_item": (I, e)}
    for k, (n_in, w) in enumerate(zip(layer_inputs(layers), layers)):
        out["kernel%d" % k], out["bias%d" % k] = (n_in, int(w)), (int(w),)
    return {n: out[n] for n in names(layers, d)}


def init_tables(U, I, d, layers, seed):
    """seeded float32 initial values: embeddings N(0, 0.3), kernels glorot-uniform, biases U(-0.1, 0.3) — the reference
    starts its biases at zero; a trace from non-zero ones also tells a dropped bias term from the first step on"""
    rs = np.random.RandomState(seed)
    out = {}
    for n, shape in shapes(U, I, d, layers).items():
        if n.startswith("kernel"):
            lim = np.sqrt(6.0 / max(shape[0] + shape[1], 1))
            out[n] = rs.uniform(-lim, lim, shape).astype(np.float32)
        elif n.startswith("bias"):
            out[n] = rs.uniform(-0.1, 0.3, shape).astype(np.float32)
        else:
            out[n] = (0.3 * rs.standard_normal(shape)).astype(np.float32)
    return out


def _f64(tab):
    return {k: np.asarray(v, dtype=np.float64) for k, v in tab.items()}


def forward(tab, users, items, layers):
    """(y [B], the activations h_{-1} .. h_last, the pre-activations) in float64"""
    tab = _f64(tab)
    users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
    h = [np.concatenate([tab["mlp_embedding_user"][users], tab["mlp_embedding_item"][items]], axis=1)]
    pre = []
    for k in range(len(layers)):
        z = h[-1] @ tab["kernel%d" % k] + tab["bias%d" % k]
        pre.append(z)
        h.append(np.maximum(z, 0.0))
    y = h[-1].sum(axis=1)
    if "mf_embedding_user" in tab:
        y = y + (tab["mf_embedding_user"][users] * tab["mf_embedding_item"][items]).sum(axis=1)
    return y, h, pre


def loss_and_dy(y, labels, loss):
    """(the data term, d term / d y): tf.losses.sigmoid_cross_entropy is the MEAN over the batch, square a sum"""
    labels = np.asarray(labels, np.float64)
    if loss == "square":
        return ((labels - y) ** 2).sum(), -2.0 * (labels - y)
    B = max(len(y), 1)
    term = np.maximum(y, 0.0) - y * labels + np.log1p(np.exp(-np.abs(y)))
    return term.sum() / B, (1.0 / (1.0 + np.exp(-y)) - labels) / B


def gradients(tab, users, items, labels, layers, loss="cross_entropy", reg_mf=0.0, reg_mlp=0.0):
    """((data term, regulariser term), {name: gradient}): the tables' gradients are the sums over the batch's
    occurrences of a row (IndexedSlices densified), the regulariser on the gathered rows"""
    tab = _f64(tab)
    users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
    y, h, pre = forward(tab, users, items, layers)
    term, dy = loss_and_dy(y, labels, loss)
    G = {k: np.zeros_like(v) for k, v in tab.items()}
    reg = 0.0
    dh = np.repeat(dy[:, None], int(layers[-1]), axis=1)
    for k in range(len(layers) - 1, -1, -1):
        dz = dh * (pre[k] > 0.0)                          # relu: 0 where the pre-activation is <= 0
        G["kernel%d" % k] = h[k].T @ dz
        G["bias%d" % k] = dz.sum(axis=0)
        dh = dz @ tab["kernel%d" % k].T
    e = int(layers[0]) // 2
    m, n = tab["mlp_embedding_user"][users], tab["mlp_embedding_item"][items]
    np.add.at(G["mlp_embedding_user"], users, dh[:, :e] + reg_mlp * m)
    np.add.at(G["mlp_embedding_item"], items, dh[:, e:] + reg_mlp * n)
    reg += reg_mlp * 0.5 * ((m * m).sum() + (n * n).sum())
    if "mf_embedding_user" in tab:
        p, q = tab["mf_embedding_user"][users], tab["mf_embedding_item"][items]
        np.add.at(G["mf_embedding_user"], users, dy[:, None] * q + reg_mf * p)
        np.add.at(G["mf_embedding_item"], items, dy[:, None] * p + reg_mf * q)
        reg += reg_mf * 0.5 * ((p * p).sum() + (q * q).sum())
    return (float(term), float(reg)), G


def total_loss(tab, users, items, labels, layers, loss, reg_mf, reg_mlp):
    """the scalar the optimiser minimises, for central differences"""
    tab = _f64(tab)
    users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
    y, _, _ = forward(tab, users, items, layers)
    out = loss_and_dy(y, labels, loss)[0]
    m, n = tab["mlp_embedding_user"][users], tab["mlp_embedding_item"][items]
    out += reg_mlp * 0.5 * ((m * m).sum() + (n * n).sum())
    if "mf_embedding_user" in tab:
        p, q = tab["mf_embedding_user"][users], tab["mf_embedding_item"][items]
        out += reg_mf * 0.5 * ((p * p).sum() + (q * q).sum())
    return float(out)


def scores(tab, users, layers):
    """[n, I]: predict() in full mode — every item for each user, the unsplit graph"""
    I = len(tab["mlp_embedding_item"])
    users = np.asarray(users, np.int64)
    return np.stack([forward(tab, np.full(I, u), np.arange(I), layers)[0] for u in users]) if len(users) else \
        np.zeros((0, I))


def scores_split(tab, users, layers):
    """the same scores the way the device scorer forms them: W1 = [W1u ; W1i], A = M_users W1u + b1 once per user, Bm =
    N W1i once per item, h_1 = relu(A_u + Bm_i) — legal because the first layer is linear in the concat before its relu"""
    tab = _f64(tab)
    users = np.asarray(users, np.int64)
    e = int(layers[0]) // 2
    W1 = tab["kernel0"]
    A = tab["mlp_embedding_user"][users] @ W1[:e] + tab["bias0"]
    Bm = tab["mlp_embedding_item"] @ W1[e:]
    h = np.maximum(A[:, None, :] + Bm[None, :, :], 0.0)
    for k in range(1, len(layers)):
        h = np.maximum(h @ tab["kernel%d" % k] + tab["bias%d" % k], 0.0)
    y = h.sum(axis=2)
    if "mf_embedding_user" in tab:
        y = y + tab["mf_embedding_user"][users] @ tab["mf_embedding_item"].T
    return y


class State:
    """the variables and their optimiser slots in float64; step() is one sess.run((loss, optimizer))"""

    def __init__(self, tab, layers, learner="adam", lr=LR, momentum=0.9):
        self.var = {k: np.array(v, dtype=np.float64) for k, v in tab.items()}
        self.layers, self.learner, self.lr, self.momentum = list(layers), learner, lr, momentum
        init = {"adam": 0.0, "gd": 0.0, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        self.s0 = {k: np.full_like(v, init) for k, v in self.var.items()}
        self.s1 = {k: np.zeros_like(v) for k, v in self.var.items()}
        self.b1p, self.b2p = 0.9, 0.999

    def apply(self, key, g, rows):
        """rows None: the dense Apply* kernel; else the sparse one on `rows` (Adam's sparse form sweeps every row)"""
        var, s0, s1, lr = self.var[key], self.s0[key], self.s1[key], self.lr
        r = slice(None) if rows is None else rows
        if self.learner == "adam":
            alpha = lr * np.sqrt(1 - self.b2p) / (1 - self.b1p)
            if rows is None:
                s0 += (g - s0) * (1 - 0.9)
                s1 += (g * g - s1) * (1 - 0.999)
                var -= (s0 * alpha) / (np.sqrt(s1) + 1e-8)
            else:
                s0[:] = s0 * 0.9 + g * (1 - 0.9)
                s1[:] = s1 * 0.999 + (g * g) * (1 - 0.999)
                var -= alpha * s0 / (np.sqrt(s1) + 1e-8)
        elif self.learner == "gd":
            var[r] -= lr * g[r]
        elif self.learner == "adagrad":
            s0[r] += g[r] * g[r]
            var[r] -= (lr * g[r]) / np.sqrt(s0[r])
        elif self.learner == "rmsprop":
            if rows is None:
                s0 += (g * g - s0) * (1 - 0.9)
                s1[:] = s1 * 0.0 + (g * lr) / np.sqrt(1e-10 + s0)
            else:
                s0[r] = s0[r] * 0.9 + (g[r] * g[r]) * (1 - 0.9)
                s1[r] = s1[r] * 0.0 + (1.0 / np.sqrt(s0[r] + 1e-10)) * lr * g[r]
            var[r] -= s1[r]
        else:
            s0[r] = s0[r] * self.momentum + g[r]
            var[r] -= s0[r] * lr

    def step(self, users, items, labels, loss, reg_mf, reg_mlp):
        """returns the pre-update (data term, regulariser term)"""
        loss2, G = gradients(self.var, users, items, labels, self.layers, loss, reg_mf, reg_mlp)
        for key in self.var:
            if key in TABLES:
                ids = users if key.endswith("user") else items
                self.apply(key, G[key], np.unique(np.asarray(ids, np.int64)))
            else:
                self.apply(key, G[key], None)
        self.b1p *= 0.9
        self.b2p *= 0.999
        return loss2
