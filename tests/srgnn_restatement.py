"""SRGNN in numpy, written from model/sequential_recommender/SRGNN.py's graph and the published definitions of its ops:
the session-graph build, the forward pass, a hand-written backward pass, the staircase schedule and TF-1.12's Adam.
`dtype` float64 gives the statement the tests call exact, float32 its twin: the distance between the two is the
yardstick of the device step's edge cases.

A batch is seq int [B, L] post-padded with an id outside [0, I) (the first such id ends the session) and target [B].
Sessions are independent, so the statement goes session by session; the pad nodes of the reference (no edges, mask 0)
take no part in any value or gradient and are left out."""
import numpy as np

NAMES = ("nasr_w1", "nasr_w2", "nasrv", "nasr_b", "embedding", "W_in", "b_in", "W_out", "b_out", "B", "gates_kernel",
         "gates_bias", "candidate_kernel", "candidate_bias")


# the golden's cases: hidden_size, step, nonhybrid, L2, max_seq_len, lr_dc (decay_steps is 2 in `hybrid`: the rate
# drops before step 3; the others never reach their first drop)
CASES = {"hybrid": (16, 1, False, 1e-5, 6, 0.1), "gated": (20, 2, True, 0.0, 8, 0.1), "repeats": (72, 3, False, 1e-5, 12, 0.1)}
LR = 0.001
PREDICT_CASE = "gated"


def shapes(I, d):
    return {"nasr_w1": (d, d), "nasr_w2": (d, d), "nasrv": (1, d), "nasr_b": (d,), "embedding": (I, d), "W_in": (d, d),
            "b_in": (d,), "W_out": (d, d), "b_out": (d,), "B": (2 * d, d), "gates_kernel": (3 * d, 2 * d),
            "gates_bias": (2 * d,), "candidate_kernel": (3 * d, d), "candidate_bias": (d,)}


def init_tables(I, d, seed=0, scale=1.0):
    """float32 values drawn as SRGNN.py:51-73 and the GRUCell draw theirs (not the plugin's stream)"""
    rs = np.random.RandomState(seed)
    stdv = 1.0 / np.sqrt(d)
    out = {}
    for name, shape in shapes(I, d).items():
        if name in ("gates_kernel", "candidate_kernel"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            out[name] = rs.uniform(-lim, lim, shape)
        else:
            out[name] = rs.uniform(-stdv, stdv, shape)
    out["nasr_b"] = np.zeros(d)
    out["gates_bias"] = np.ones(2 * d)
    out["candidate_bias"] = np.zeros(d)
    out["embedding"] = out["embedding"] * scale
    return {k: v.astype(np.float32) for k, v in out.items()}


def session_of(row, I):
    """the items of one padded row: up to the first id outside [0, I)"""
    out = []
    for x in row:
        if not 0 <= x < I:
            break
        out.append(int(x))
    return out


def build_graph(items, dtype=np.float64):
    """SRGNN._build_session_graph (SRGNN.py:176-205) for one session, without pad nodes: nodes (ascending distinct ids),
    alias [len], A_in and A_out [n, n]"""
    nodes = sorted(set(items))
    idx = {v: k for k, v in enumerate(nodes)}
    alias = [idx[v] for v in items]
    n = len(nodes)
    adj = np.zeros((n, n))
    for t in range(len(items) - 1):
        adj[alias[t], alias[t + 1]] = 1                       # a repeated edge stays 1
    s_in = adj.sum(0)
    s_in[s_in == 0] = 1
    s_out = adj.sum(1)
    s_out[s_out == 0] = 1
    a_in = adj / s_in                                         # the divisor is indexed by the column in both
    a_out = adj.T / s_out
    return nodes, alias, a_in.astype(np.float32).astype(dtype), a_out.astype(np.float32).astype(dtype)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _forward_session(V, items, step, nonhybrid, dtype):
    d = V["nasr_w1"].shape[0]
    nodes, alias, a_in, a_out = build_graph(items, dtype)
    h = V["embedding"][nodes] if nodes else np.zeros((0, d), dtype)
    saved = []
    Wg, Wc = V["gates_kernel"], V["candidate_kernel"]
    for _ in range(step):
        fi = h @ V["W_in"] + V["b_in"]
        fo = h @ V["W_out"] + V["b_out"]
        x = np.concatenate([a_in @ fi, a_out @ fo], 1)
        g = _sigmoid(np.concatenate([x, h], 1) @ Wg + V["gates_bias"])
        r, u = g[:, :d], g[:, d:]                             # r first, u second
        c = np.tanh(np.concatenate([x, r * h], 1) @ Wc + V["candidate_bias"])     # r * s before the product
        saved.append((h, x, r, u, c))
        h = u * h + (1 - u) * c
    n_t = len(items)
    seq_h = h[alias] if n_t else np.zeros((0, d), dtype)
    last_h = h[alias[-1]] if n_t else np.zeros(d, dtype)
    last = last_h @ V["nasr_w1"]
    m = _sigmoid(last + seq_h @ V["nasr_w2"] + V["nasr_b"])
    coef = m @ V["nasrv"][0]                                  # the mask is 1 on every position kept here
    a = coef @ seq_h
    ma = np.concatenate([a, last])
    sess = a if nonhybrid else ma @ V["B"]
    return sess, (nodes, alias, a_in, a_out, saved, h, seq_h, last_h, last, m, coef, a, ma)


def forward(V, seq, step, nonhybrid=False, dtype=np.float64):
    """the session embeddings [B, d]"""
    V = {k: np.asarray(v, dtype) for k, v in V.items()}
    I = V["embedding"].shape[0]
    return np.stack([_forward_session(V, session_of(row, I), step, nonhybrid, dtype)[0] for row in seq]).astype(dtype)


def logits(V, seq, step, nonhybrid=False, dtype=np.float64):
    return forward(V, seq, step, nonhybrid, dtype) @ np.asarray(V["embedding"], dtype).T


def loss_and_grads(V, seq, target, step, L2, nonhybrid=False, dtype=np.float64):
    """(cross-entropy mean, regulariser term, {name: gradient of their sum})"""
    V = {k: np.asarray(v, dtype) for k, v in V.items()}
    emb = V["embedding"]
    I, d = emb.shape
    Bn = len(seq)
    G = {k: np.zeros_like(v) for k, v in V.items()}
    Wg, Wc = V["gates_kernel"], V["candidate_kernel"]
    ce = dtype(0)
    for row, tar in zip(seq, target):
        items = session_of(row, I)
        sess, (nodes, alias, a_in, a_out, saved, h, seq_h, last_h, last, m, coef, a, ma) = \
            _forward_session(V, items, step, nonhybrid, dtype)
        z = emb @ sess
        zmax = z.max()
        e = np.exp(z - zmax)
        lse = np.log(e.sum()) + zmax
        ce += lse - z[tar]
        dl = e / e.sum()
        dl[tar] -= 1
        dl = dl / dtype(Bn)                                   # the mean over the batch
        G["embedding"] += np.outer(dl, sess)
        dsess = dl @ emb
        if nonhybrid:
            da, dlast = dsess, np.zeros(d, dtype)
        else:
            G["B"] += np.outer(ma, dsess)
            dma = V["B"] @ dsess
            da, dlast = dma[:d], dma[d:].copy()
        dcoef = seq_h @ da
        dseq_h = np.outer(coef, da)
        G["nasrv"][0] += dcoef @ m
        dpre = dcoef[:, None] * V["nasrv"][0] * m * (1 - m)
        G["nasr_b"] += dpre.sum(0)
        dlast = dlast + dpre.sum(0)
        G["nasr_w2"] += seq_h.T @ dpre
        dseq_h += dpre @ V["nasr_w2"].T
        G["nasr_w1"] += np.outer(last_h, dlast)
        dh = np.zeros_like(h)
        for t, k in enumerate(alias):
            dh[k] += dseq_h[t]
        if items:
            dh[alias[-1]] += V["nasr_w1"] @ dlast
        for s, x, r, u, c in reversed(saved):
            du, dc = dh * (s - c), dh * (1 - u)
            ds = dh * u                                       # through u s
            dpc = dc * (1 - c * c)
            xc = np.concatenate([x, r * s], 1)
            G["candidate_kernel"] += xc.T @ dpc
            G["candidate_bias"] += dpc.sum(0)
            dxc = dpc @ Wc.T
            dx, drs = dxc[:, :2 * d], dxc[:, 2 * d:]          # the candidate kernel's state rows
            ds += drs * r                                     # through r s
            dpg = np.concatenate([drs * s * r * (1 - r), du * u * (1 - u)], 1)
            G["gates_kernel"] += np.concatenate([x, s], 1).T @ dpg
            G["gates_bias"] += dpg.sum(0)
            dxg = dpg @ Wg.T
            dx = dx + dxg[:, :2 * d]
            ds += dxg[:, 2 * d:]                              # the gate kernel's state rows
            dfi, dfo = a_in.T @ dx[:, :d], a_out.T @ dx[:, d:]
            G["W_in"] += s.T @ dfi
            G["b_in"] += dfi.sum(0)
            G["W_out"] += s.T @ dfo
            G["b_out"] += dfo.sum(0)
            dh = ds + dfi @ V["W_in"].T + dfo @ V["W_out"].T
        for k, node in enumerate(nodes):
            G["embedding"][node] += dh[k]
    ce = ce / dtype(Bn)
    reg = dtype(0)
    for k in NAMES:                                           # the name filter of SRGNN.py:135 removes nothing
        reg += dtype(L2) * (V[k] * V[k]).sum() / 2
        G[k] += dtype(L2) * V[k]
    return ce, reg, G


def learning_rates(lr, lr_dc, decay_steps, n_steps, first=0):
    """tf.train.exponential_decay(staircase=True) in float32, for global_step first .. first + n_steps - 1"""
    out = np.zeros(n_steps, np.float32)
    for k in range(n_steps):
        p = np.floor(np.float32(first + k) / np.float32(decay_steps))
        out[k] = np.float32(lr) * np.power(np.float32(lr_dc), p, dtype=np.float32)
    return out


class Adam:
    """TF-1.12 ApplyAdam: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); v -= lr_t m / (sqrt(v) + eps)"""

    def __init__(self, V, dtype=np.float64, b1=0.9, b2=0.999, eps=1e-8):
        self.dtype, self.b1, self.b2, self.eps = dtype, dtype(b1), dtype(b2), dtype(eps)
        self.m = {k: np.zeros_like(np.asarray(v, dtype)) for k, v in V.items()}
        self.v = {k: np.zeros_like(np.asarray(v, dtype)) for k, v in V.items()}
        self.b1p, self.b2p = self.b1, self.b2

    def apply(self, V, G, lr):
        one = self.dtype(1)
        alpha = self.dtype(lr) * np.sqrt(one - self.b2p) / (one - self.b1p)
        for k in V:
            self.m[k] += (G[k] - self.m[k]) * (one - self.b1)
            self.v[k] += (G[k] * G[k] - self.v[k]) * (one - self.b2)
            V[k] = V[k] - alpha * self.m[k] / (np.sqrt(self.v[k]) + self.eps)
        self.b1p, self.b2p = self.b1p * self.b1, self.b2p * self.b2


def train(V, feeds, step, L2, lrs, nonhybrid=False, dtype=np.float64):
    """feeds: [(seq, target)]; returns (losses, the variables after each step)"""
    V = {k: np.array(v, dtype) for k, v in V.items()}
    adam = Adam(V, dtype)
    losses, trace = [], []
    for (seq, target), lr in zip(feeds, lrs):
        ce, reg, G = loss_and_grads(V, seq, target, step, L2, nonhybrid, dtype)
        adam.apply(V, G, lr)
        losses.append(ce + reg)
        trace.append({k: v.copy() for k, v in V.items()})
    return losses, trace
