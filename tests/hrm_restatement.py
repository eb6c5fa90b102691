"""A float64 numpy restatement of HRM (model/sequential_recommender/HRM.py:62-95, util/learner.py, TF-1.12's sparse
optimiser kernels) for the HRM tests: one training step for every aggregation pair, loss and learner, predict() with
the reference's slice quirk and the two stated deviations, and the tie rule of the max's gradient written out: the
derivative of a column goes to the inputs EQUAL to the maximum, in equal shares (TF's _MinOrMaxGrad: indicators /
num_selected * grad).  Checked against the reference class's own f64 trace in test_hrm_cpu.py; the GPU tests use it
for the shapes the trace does not hold.  `gradients` computes in the dtype of the tables it is given, so that the
constructed-ties test can run it in float32 as well."""
import numpy as np

import fism_restatement as F

TABLES = ("P", "V")
# case -> (loss, learner, pre_agg, session_agg, high_order)
CASES = {"ce_adam_max_max": ("cross_entropy", "adam", "max", "max", 3),
         "ce_adam_max_avg": ("cross_entropy", "adam", "max", "avg", 3),
         "ce_adam_avg_max": ("cross_entropy", "adam", "avg", "max", 3),
         "ce_adam_avg_avg": ("cross_entropy", "adam", "avg", "avg", 3),
         "square_adam": ("square", "adam", "max", "max", 2), "square_gd": ("square", "gd", "max", "max", 2),
         "square_adagrad": ("square", "adagrad", "max", "max", 2),
         "square_rmsprop": ("square", "rmsprop", "max", "max", 2),
         "square_momentum": ("square", "momentum", "max", "max", 2),
         "one_max": ("cross_entropy", "adam", "max", "max", 1), "one_avg": ("cross_entropy", "adam", "avg", "max", 1)}
PREDICT_CASE = "ce_adam_max_max"


class State(F.State):
    """the optimiser state of fism_restatement on HRM's two tables; both get the sparse application"""

    def __init__(self, P, V, learner="adam", lr=0.01, momentum=0.9):
        f = lambda x: np.array(x, dtype=np.float64)
        self.var = {"P": f(P), "V": f(V)}
        self.learner, self.lr, self.momentum = learner, lr, momentum
        init = {"adam": 0.0, "gd": 0.0, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        self.s0 = {k: np.full_like(v, init) for k, v in self.var.items()}
        self.s1 = {k: np.zeros_like(v) for k, v in self.var.items()}
        self.b1p, self.b2p = 0.9, 0.999


def golden_tables(g, case, tag, step):
    """(P, V) of the trace after `step` (0-based; -1: the initial tables), full size, in the trace's width"""
    dt = np.float32 if tag == "f32" else np.float64
    out = []
    for name in TABLES:
        t = g[name + "_0"].astype(np.float64)
        if step >= 0:
            rows = g["%s_rows_%s" % (case, name)]
            t[rows] = t[rows] + g["%s_%s_%s" % (case, tag, name)][step]
        out.append(t.astype(dt))
    return out


def sequences(g):
    """{user: [items by time]} of the golden's train pattern"""
    ptr, seq = g["seq_ptr"], g["seq"]
    return {u: seq[ptr[u]:ptr[u + 1]].tolist() for u in range(len(ptr) - 1) if ptr[u + 1] > ptr[u]}


# ------------------------------------------------------------------ the two poolings and their shares
def pool_session(rows, use_max):
    """rows [N, m, d] -> (s [N, d], w [N, m, d]): w[n, l, c] = d s[n, c] / d rows[n, l, c].  One row is that row
    (HRM.py:75-77 at high_order = 1; a max or a mean over one row otherwise)."""
    one = rows.dtype.type(1)
    m = rows.shape[1]
    if m == 1:
        return rows[:, 0], np.ones_like(rows)
    if use_max:
        s = rows.max(axis=1)
        tied = (rows == s[:, None, :]).astype(rows.dtype)          # the inputs equal to the maximum ...
        return s, tied / tied.sum(axis=1, keepdims=True)          # ... share its derivative equally
    return rows.sum(axis=1) / rows.dtype.type(m), np.full_like(rows, one) / rows.dtype.type(m)


def pool_pre(p, s, use_max):
    """p, s [N, d] -> (h, share of p, share of s)"""
    half = p.dtype.type(0.5)
    if use_max:
        h = np.maximum(p, s)
        tp, ts = (p == h).astype(p.dtype), (s == h).astype(p.dtype)
        return h, tp / (tp + ts), ts / (tp + ts)                  # a tie: one half each
    return (p + s) / p.dtype.type(2), np.full_like(p, half), np.full_like(p, half)


def tie_counts(P, V, users, recents, pre_agg, session_agg):
    """(columns in which two or more recents hold the session max, columns in which P[u] equals the session row) over
    the batch, on the tables as they come in"""
    rec = np.asarray(recents, np.int64).reshape(len(users), -1)
    rows = V[rec]
    s, _ = pool_session(rows, session_agg == "max")
    n_sess = int(((rows == s[:, None, :]).sum(axis=1) >= 2).sum()) if rec.shape[1] > 1 else 0
    return n_sess, int((P[np.asarray(users, np.int64)] == s).sum())


def gradients(P, V, users, recents, items, labels, loss, reg, pre_agg, session_agg):
    """(loss, G_P, G_V) of one batch in the dtype of P: HRM.py:62-91 and its derivative"""
    dt = P.dtype.type
    u, i = np.asarray(users, np.int64), np.asarray(items, np.int64)
    rec = np.asarray(recents, np.int64).reshape(len(u), -1)
    N, L = rec.shape
    p, q, rows = P[u], V[i], V[rec]
    s, w = pool_session(rows, session_agg == "max")
    h, share_p, share_s = pool_pre(p, s, pre_agg == "max")
    x = (h * q).sum(axis=1)
    y = np.asarray(labels, P.dtype)
    if loss == "square":
        total, g = ((y - x) ** 2).sum(), dt(-2) * (y - x)
    else:
        total = (np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).mean() if N else dt(0)
        g = (dt(1) / (dt(1) + np.exp(-x)) - y) / dt(max(N, 1))
    total = total + dt(reg) * dt(0.5) * ((p ** 2).sum() + (rows ** 2).sum() + (q ** 2).sum())   # per occurrence
    GP, GV = np.zeros_like(P), np.zeros_like(V)
    dh = g[:, None] * q
    np.add.at(GP, u, dh * share_p + dt(reg) * p)
    np.add.at(GV, i, g[:, None] * h + dt(reg) * q)
    ds = dh * share_s
    np.add.at(GV, rec.reshape(-1), (ds[:, None, :] * w + dt(reg) * rows).reshape(N * L, -1))
    return total, GP, GV


def step(st, users, recents, items, labels, loss, reg, pre_agg, session_agg):
    """one sess.run((loss, optimizer)): returns the pre-update loss"""
    total, GP, GV = gradients(st.var["P"], st.var["V"], users, recents, items, labels, loss, reg, pre_agg, session_agg)
    st.apply("P", GP, np.unique(np.asarray(users, np.int64)))
    st.apply("V", GV, np.unique(np.concatenate([np.asarray(items, np.int64).reshape(-1),
                                                np.asarray(recents, np.int64).reshape(-1)])))
    st.b1p, st.b2p = st.b1p * 0.9, st.b2p * 0.999
    return float(total)


# ------------------------------------------------------------------ predict
def last_items_table(seqs, n_users, L):
    """int32 [U, L]: what HRM.py:144 feeds — `seq[len(seq) - L:]`; for 0 < |R_u| < L the start is negative and the
    slice holds the last min(L - |R_u|, |R_u|) items.  -1 elsewhere, and in the rows of users without train items."""
    last = np.full((n_users, L), -1, np.int32)
    for u, s in seqs.items():
        n = len(s)
        m = min(L, n) if n >= L else min(L - n, n)
        if m:
            last[u, :m] = s[n - m:]
    return last


def user_factors(P, V, users, last, pre_agg, session_agg):
    """h_u [n, d]: pooled over the user's valid last items; none (deviation a): P[u] alone.  At L = 1 (deviation b) the
    user is pooled with its last item, as in training."""
    P, V = np.asarray(P, np.float64), np.asarray(V, np.float64)
    out = np.empty((len(users), P.shape[1]))
    for k, u in enumerate(users):
        tail = [int(r) for r in last[u] if r >= 0]
        if not tail:
            out[k] = P[u]
            continue
        s, _ = pool_session(V[tail][None], session_agg == "max")
        out[k] = pool_pre(P[u][None], s, pre_agg == "max")[0][0]
    return out


def predict(P, V, users, last, pre_agg, session_agg):
    """HRM.py:135-163: every item against h_u"""
    return user_factors(P, V, users, last, pre_agg, session_agg) @ np.asarray(V, np.float64).T


def edge_patterns(users, recents, items):
    """the duplicate patterns a golden batch holds: a user twice; an item that is the target of one instance and a
    recent of another"""
    users, items = np.asarray(users).tolist(), np.asarray(items).tolist()
    return {"user twice": len(set(users)) < len(users),
            "recent and target": bool(set(np.asarray(recents).reshape(-1).tolist()) & set(items))}
