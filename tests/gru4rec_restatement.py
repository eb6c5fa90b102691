"""A numpy restatement of GRU4Rec (model/sequential_recommender/GRU4Rec.py, TF-1.12's GRUCell and Adam kernels) for
the GRU4Rec tests, in float64 or — the same code, `dtype=np.float32` — in float32: the cell, one step with its analytic
gradients, TF's two Adam forms, the session-parallel epoch loop (written from the reference's loop, independently of the
plugin's schedule function), the users' final states and predict().  Checked against the reference class's own f64 trace
in test_gru4rec_cpu.py; the GPU tests use it for the shapes the trace does not hold, and its float32 run as the
yardstick of what float32 can reach on a long sequence."""
import numpy as np

# case -> (loss, hidden_act, final_act, layers, reg)
CASES = {"top1_tanh_linear": ("top1", "tanh", "linear", [16], 0.0),
         "bpr_relu_leaky": ("bpr", "relu", "leaky_relu", [24, 8], 0.01),
         "top1_tanh_relu": ("top1", "tanh", "relu", [8, 8, 8], 0.01)}
PREDICT_CASE = "top1_tanh_linear"
LR = 0.001
LEAKY = 0.2


def table_names(n_layers):
    """the variables in creation order"""
    out = ["E_in", "Q", "b"]
    for l in range(n_layers):
        out += ["Wg%d" % l, "bg%d" % l, "Wc%d" % l, "bc%d" % l]
    return out


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def hidden(act, x):
    return np.maximum(x, 0) if act == "relu" else np.tanh(x)


def hidden_grad(act, c):
    return (c > 0).astype(c.dtype) if act == "relu" else 1 - c * c


def final(act, z):
    if act == "relu":
        return np.maximum(z, 0)
    if act == "leaky_relu":
        return np.maximum(z * z.dtype.type(LEAKY), z)
    return z


def final_grad(act, z):
    one = z.dtype.type(1)
    if act == "relu":
        return (z > 0).astype(z.dtype)
    if act == "leaky_relu":
        return np.where(z > 0, one, z.dtype.type(LEAKY))
    return np.ones_like(z)


def cell(x, s, Wg, bg, Wc, bc, act):
    """[EXT: tensorflow r1.12 rnn_cell_impl.GRUCell.call] -> (h, (r, u, c))"""
    n = s.shape[1]
    g = sigmoid(np.concatenate([x, s], axis=1) @ Wg + bg)
    r, u = g[:, :n], g[:, n:]
    c = hidden(act, np.concatenate([x, r * s], axis=1) @ Wc + bc)
    return u * s + (1 - u) * c, (r, u, c)


def forward(V, X, states, hidden_act):
    """the stack on E_in[X]: (new states [h_l], per-layer caches)"""
    x = V["E_in"][np.asarray(X, np.int64)]
    hs, caches = [], []
    for l, s in enumerate(states):
        h, (r, u, c) = cell(x, s, V["Wg%d" % l], V["bg%d" % l], V["Wc%d" % l], V["bc%d" % l], hidden_act)
        caches.append((x, s, r, u, c))
        hs.append(h)
        x = h
    return hs, caches


def loss_and_dlogits(A, loss):
    """(loss, dLoss/dA) of GRU4Rec.py:87-101 on the activated logits A [B, B]"""
    B = A.shape[0]
    dt = A.dtype.type
    p = np.diag(A)[:, None]
    inv = dt(1) / (dt(B) * dt(B))
    eye = np.eye(B, dtype=A.dtype)
    if loss == "bpr":
        y = p - A
        total = (np.maximum(-y, 0) + np.log1p(np.exp(-np.abs(y)))).sum() * inv
        e = sigmoid(-y)
        dA = e * inv - eye * (e.sum(axis=1, keepdims=True) * inv)
    else:
        e, q = sigmoid(A - p), sigmoid(A * A)
        qp = sigmoid(p * p)
        total = ((e + q).sum() - qp.sum()) * inv
        de = e * (1 - e)
        dA = (de + 2 * A * q * (1 - q)) * inv
        dA = dA - eye * ((de.sum(axis=1, keepdims=True) + 2 * p * qp * (1 - qp)) * inv)
    return total, dA


def gradients(V, X, Y, states, loss, hidden_act, final_act, reg):
    """((loss term, regulariser term), {variable: gradient}, new states) of one step: GRU4Rec.py:111-131 and its
    derivative by hand.  The states are constants; the regulariser is on the GATHERED rows: a duplicate counts per slot"""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    dt = V["E_in"].dtype.type
    L = len(states)
    hs, caches = forward(V, X, states, hidden_act)
    top = hs[-1]
    Qy, by = V["Q"][Y], V["b"][Y]
    Z = top @ Qy.T + by[None, :]
    total, dA = loss_and_dlogits(final(final_act, Z), loss)
    dZ = dA * final_grad(final_act, Z)
    x0 = caches[0][0]
    l2 = dt(0.5) * ((x0 * x0).sum() + (Qy * Qy).sum() + (by * by).sum())
    G = {k: np.zeros_like(v) for k, v in V.items()}
    np.add.at(G["Q"], Y, dZ.T @ top + dt(reg) * Qy)
    np.add.at(G["b"], Y, dZ.sum(axis=0) + dt(reg) * by)
    dh = dZ @ Qy
    for l in range(L - 1, -1, -1):
        x, s, r, u, c = caches[l]
        Wg, Wc = V["Wg%d" % l], V["Wc%d" % l]
        n_in = x.shape[1]
        dpc = dh * (1 - u) * hidden_grad(hidden_act, c)
        dpu = dh * (s - c) * u * (1 - u)
        drs = dpc @ Wc[n_in:].T
        dpr = drs * s * r * (1 - r)
        dpg = np.concatenate([dpr, dpu], axis=1)
        G["Wc%d" % l] = np.concatenate([x, r * s], axis=1).T @ dpc
        G["bc%d" % l] = dpc.sum(axis=0)
        G["Wg%d" % l] = np.concatenate([x, s], axis=1).T @ dpg
        G["bg%d" % l] = dpg.sum(axis=0)
        dh = dpc @ Wc[:n_in].T + dpg @ Wg[:n_in].T
    np.add.at(G["E_in"], X, dh + dt(reg) * x0)
    return (total, dt(reg) * l2), G, hs


class State:
    """the variables, Adam's slots and beta powers, and the recurrent states"""

    def __init__(self, V, layers, batch, lr=LR, dtype=np.float64):
        self.dtype = dtype
        self.V = {k: np.array(v, dtype=dtype) for k, v in V.items()}
        self.m = {k: np.zeros_like(v) for k, v in self.V.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.V.items()}
        self.layers = list(layers)
        self.states = [np.zeros((batch, n), dtype=dtype) for n in layers]
        t = dtype
        self.lr, self.b1, self.b2, self.eps = t(lr), t(0.9), t(0.999), t(1e-8)
        self.b1p, self.b2p = t(0.9), t(0.999)

    def apply(self, G):
        """python/training/adam.py [EXT]: E_in, Q and b are read through gathers only -> _apply_sparse_shared (every
        row decays, the summed slices are added); the cells' variables -> ApplyAdam"""
        one = self.dtype(1)
        alpha = self.lr * np.sqrt(one - self.b2p) / (one - self.b1p)
        for k, g in G.items():
            m, v = self.m[k], self.v[k]
            if k in ("E_in", "Q", "b"):
                m *= self.b1
                m += g * (one - self.b1)
                v *= self.b2
                v += (g * g) * (one - self.b2)
                self.V[k] = self.V[k] - alpha * m / (np.sqrt(v) + self.eps)
            else:
                m += (g - m) * (one - self.b1)
                v += (g * g - v) * (one - self.b2)
                self.V[k] = self.V[k] - (m * alpha) / (np.sqrt(v) + self.eps)
        self.b1p, self.b2p = self.b1p * self.b1, self.b2p * self.b2


def step(st, X, Y, loss, hidden_act, final_act, reg, reset=None):
    """one sess.run([update_opt, final_state]) with the states fed from `st`, then the hand-over and the reset mask
    (GRU4Rec.py:160, 172-174): returns (loss term, regulariser term)"""
    losses, G, hs = gradients(st.V, X, Y, st.states, loss, hidden_act, final_act, reg)
    st.apply(G)
    st.states = [h.copy() for h in hs]
    if reset is not None:
        mask = np.asarray(reset).astype(bool)
        for s in st.states:
            s[mask] = 0
    return losses


def epoch_feeds(offset_idx, data_items, user_idx, batch_size):
    """GRU4Rec.py:141-174 as a generator of (in_idx, out_idx, zero_on_entry [B] bool): the loop of the reference with
    the session call taken out; zero_on_entry marks the state rows that are zero when the step is fed because their
    slot was (re)filled — every row at the first step"""
    iters = np.arange(batch_size, dtype=np.int32)
    maxiter = iters.max()
    start = offset_idx[user_idx[iters]]
    end = offset_idx[user_idx[iters] + 1]
    zero = np.ones(batch_size, bool)
    finished = False
    while not finished:
        min_len = (end - start).min()
        out_idx = data_items[start]
        for i in range(min_len - 1):
            in_idx = out_idx
            out_idx = data_items[start + i + 1]
            yield in_idx, out_idx, zero.copy()
            zero[:] = False
        start = start + min_len - 1
        mask = np.arange(len(iters))[(end - start) <= 1]
        for idx in mask:
            maxiter += 1
            if maxiter >= len(offset_idx) - 1:
                finished = True
                break
            iters[idx] = maxiter
            start[idx] = offset_idx[user_idx[maxiter]]
            end[idx] = offset_idx[user_idx[maxiter] + 1]
        if len(mask):
            zero[mask] = True


def user_states(V, layers, hidden_act, seq_ptr, seq, users, dtype=np.float64):
    """GRU4Rec.py:179-225 per user: the top layer's output after the user's items went through the stack from a zero
    state; no items: zeros"""
    Vd = {k: np.asarray(v, dtype=dtype) for k, v in V.items()}
    out = np.zeros((len(users), layers[-1]), dtype=dtype)
    for row, u in enumerate(users):
        states = [np.zeros((1, n), dtype=dtype) for n in layers]
        for item in seq[seq_ptr[u]:seq_ptr[u + 1]]:
            states, _ = forward(Vd, [item], states, hidden_act)
        out[row] = states[-1][0]
    return out


def predict(H, Q, b, final_act):
    """GRU4Rec.py:232-250"""
    return final(final_act, H @ Q.T + b[None, :])


def init_tables(n_items, layers, seed, dtype=np.float32):
    """test tables: small random embeddings, a non-zero b, Glorot-sized kernels, gate bias one"""
    rs = np.random.RandomState(seed)
    V = {"E_in": 0.1 * rs.randn(n_items, layers[0]), "Q": 0.1 * rs.randn(n_items, layers[-1]),
         "b": 0.1 * rs.randn(n_items)}
    n_in = layers[0]
    for l, n in enumerate(layers):
        lim = np.sqrt(6.0 / (n_in + n + 2 * n))
        V["Wg%d" % l] = rs.uniform(-lim, lim, (n_in + n, 2 * n))
        V["bg%d" % l] = np.ones(2 * n) + 0.05 * rs.randn(2 * n)
        lim = np.sqrt(6.0 / (n_in + n + n))
        V["Wc%d" % l] = rs.uniform(-lim, lim, (n_in + n, n))
        V["bc%d" % l] = 0.05 * rs.randn(n)
        n_in = n
    return {k: v.astype(dtype) for k, v in V.items()}
