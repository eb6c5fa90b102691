"""A numpy restatement of GRU4RecPlus (model/sequential_recommender/GRU4RecPlus.py) for the GRU4RecPlus tests, in
float64 or — the same code, a float32 input — in float32: the row loss on the B x (B + n_sample) block with its analytic
gradients (the softmax weights differentiated), one step, and the sampler.  The cell, the stack's backward pass, TF's
two Adam forms, the epoch loop, the users' final states and predict() are gru4rec_restatement's.  Checked against the
reference class's own f64 trace in test_gru4recplus_cpu.py; the GPU tests use it for the shapes the trace does not hold."""
import numpy as np

from gru4rec_restatement import (LR, State, epoch_feeds, final, final_grad, forward, hidden_grad, init_tables,  # noqa: F401
                                 predict, sigmoid, table_names, user_states)

# case -> (loss, hidden_act, final_act, layers, reg, bpr_reg, n_sample)
CASES = {"bprmax_tanh_linear": ("bpr_max", "tanh", "linear", [16], 0.0, 1.0, 12),
         "top1max_relu_leaky": ("top1_max", "relu", "leaky_relu", [12, 8], 0.01, 1.0, 12),
         "bprmax_tanh_relu": ("bpr_max", "tanh", "relu", [8, 8, 8], 0.01, 0.5, 12),
         "top1max_tanh_linear_ns0": ("top1_max", "tanh", "linear", [8], 0.0, 1.0, 0)}
PREDICT_CASE = "bprmax_tanh_linear"
EPS = 1e-24


def softmax_neg(A):
    """GRU4RecPlus.py:91-98: (s, hm); the masked diagonal takes part in the max as a 0"""
    B, M = A.shape
    hm = 1 - np.eye(B, M, dtype=A.dtype)
    masked = A * hm
    e = np.exp(masked - masked.max(axis=1, keepdims=True)) * hm
    return e / e.sum(axis=1, keepdims=True), hm


def loss_and_dlogits(A, loss, bpr_reg):
    """(loss, dLoss/dA) of GRU4RecPlus.py:100-120 on the activated logits A [B, M]; the shift of the softmax cancels"""
    B, M = A.shape
    dt = A.dtype.type
    s, hm = softmax_neg(A)
    p = A[np.arange(B), np.arange(B)][:, None]
    eye = np.eye(B, M, dtype=A.dtype)
    if loss == "bpr_max":
        f = sigmoid(p - A)
        P = (s * f).sum(axis=1, keepdims=True)
        R = (s * A * A).sum(axis=1, keepdims=True)
        den = P + dt(EPS)
        rows = -np.log(den) + dt(bpr_reg) * R
        c = -f / den + dt(bpr_reg) * A * A                  # dL_i / ds_j
        df = s * f * (1 - f) / den
        direct = df + dt(bpr_reg) * s * 2 * A
        dp = -df.sum(axis=1, keepdims=True)
    else:
        e, q = sigmoid(A - p), sigmoid(A * A)
        g = e + q
        rows = (s * g).sum(axis=1, keepdims=True)
        c = g
        de = s * e * (1 - e)
        direct = de + s * 2 * A * q * (1 - q)
        dp = -de.sum(axis=1, keepdims=True)
    C = (s * c).sum(axis=1, keepdims=True)
    dA = (s * (c - C) + direct) * hm + eye * dp
    return rows.sum() / dt(B), dA / dt(B)


def gradients(V, X, Y, states, loss, hidden_act, final_act, reg, bpr_reg):
    """((loss term, regulariser term), {variable: gradient}, new states) of one step: GRU4RecPlus.py:130-150 and its
    derivative by hand.  Y: the len(X) positives, then the shared negatives.  The states are constants; the regulariser
    is on the GATHERED rows: a duplicate counts per slot"""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    dt = V["E_in"].dtype.type
    L = len(states)
    hs, caches = forward(V, X, states, hidden_act)
    top = hs[-1]
    Qy, by = V["Q"][Y], V["b"][Y]
    Z = top @ Qy.T + by[None, :]
    total, dA = loss_and_dlogits(final(final_act, Z), loss, bpr_reg)
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


def step(st, X, Y, loss, hidden_act, final_act, reg, bpr_reg, reset=None):
    """one sess.run([update_opt, final_state]) with the states fed from `st` (gru4rec_restatement.State), then the
    hand-over and the reset mask (GRU4RecPlus.py:186, 198-200): returns (loss term, regulariser term)"""
    losses, G, hs = gradients(st.V, X, Y, st.states, loss, hidden_act, final_act, reg, bpr_reg)
    st.apply(G)
    st.states = [h.copy() for h in hs]
    if reset is not None:
        mask = np.asarray(reset).astype(bool)
        for s in st.states:
            s[mask] = 0
    return losses


def pop_cumsum(data_items, sample_alpha):
    """GRU4RecPlus.py:59-62: counts of the items that OCCUR, in sorted item order"""
    counts = np.bincount(np.asarray(data_items, np.int64))
    pop = np.power(counts[counts > 0], sample_alpha)
    cs = np.cumsum(pop)
    return cs / cs[-1]


def epoch_feeds_plus(offset_idx, data_items, user_idx, batch_size, cumsum, n_sample):
    """GRU4RecPlus.py:163-200 as a generator of (in_idx, out_items, zero_on_entry): the reference's loop
    (gru4rec_restatement.epoch_feeds) with one np.random.rand(n_sample) per step from the global stream, the sampled
    RANKS appended as they are"""
    for in_idx, out_idx, zero in epoch_feeds(offset_idx, data_items, user_idx, batch_size):
        out_items = out_idx
        if n_sample:
            out_items = np.hstack([out_items, np.searchsorted(cumsum, np.random.rand(n_sample))])
        yield in_idx, out_items, zero
