"""A float64 numpy restatement of NPE (model/sequential_recommender/NPE.py:54-75, util/learner.py, TF-1.12's sparse
optimiser kernels) for the NPE tests: one training step for both losses and every learner, predict() with the
reference's slice quirk and the two stated deviations, and the ReLU gate written out: strict, as TF's ReluGrad
(features > 0) — an input that is exactly 0, or -0, passes nothing.  Checked against the reference class's own f64 trace
in test_npe_cpu.py; the GPU tests use it for the shapes the trace does not hold.  `gradients` computes in the dtype of
the tables it is given, so that the constructed exact case can run it in float32 as well."""
import numpy as np

import fism_restatement as F
from hrm_restatement import last_items_table, sequences          # noqa: F401  (the same slice, the same layout)

TABLES = ("P", "V", "W")
# case -> (loss, learner, high_order)
CASES = {"ce_adam": ("cross_entropy", "adam", 3), "square_adam": ("square", "adam", 3),
         "square_gd": ("square", "gd", 3), "square_adagrad": ("square", "adagrad", 3),
         "square_rmsprop": ("square", "rmsprop", 3), "square_momentum": ("square", "momentum", 3),
         "ce_adam_L2": ("cross_entropy", "adam", 2), "ce_adam_L5": ("cross_entropy", "adam", 5)}
PREDICT_CASE = "ce_adam"


class State(F.State):
    """the optimiser state of fism_restatement on NPE's three tables; all get the sparse application"""

    def __init__(self, P, V, W, learner="adam", lr=0.01, momentum=0.9):
        f = lambda x: np.array(x, dtype=np.float64)
        self.var = {"P": f(P), "V": f(V), "W": f(W)}
        self.learner, self.lr, self.momentum = learner, lr, momentum
        init = {"adam": 0.0, "gd": 0.0, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        self.s0 = {k: np.full_like(v, init) for k, v in self.var.items()}
        self.s1 = {k: np.zeros_like(v) for k, v in self.var.items()}
        self.b1p, self.b2p = 0.9, 0.999


def golden_tables(g, case, tag, step):
    """(P, V, W) of the trace after `step` (0-based; -1: the initial tables), full size, in the trace's width"""
    dt = np.float32 if tag == "f32" else np.float64
    out = []
    for name in TABLES:
        t = g[name + "_0"].astype(np.float64)
        if step >= 0:
            rows = g["%s_rows_%s" % (case, name)]
            t[rows] = t[rows] + g["%s_%s_%s" % (case, tag, name)][step]
        out.append(t.astype(dt))
    return out


# ------------------------------------------------------------------ the gate
def relu(x):
    """TF's Relu: strictly positive inputs pass"""
    return np.where(x > 0, x, x.dtype.type(0))


def gate(x):
    """TF's ReluGrad indicator: features > 0 — 0 and -0 pass nothing"""
    return (x > 0).astype(x.dtype)


def context(W, rec):
    """s [N, d]: the W rows of rec [N, L] added in l order"""
    s = np.zeros((rec.shape[0], W.shape[1]), W.dtype)
    for l in range(rec.shape[1]):
        s = s + W[rec[:, l]]
    return s


def zero_counts(P, V, W, users, recents, items):
    """(columns with P[u] == 0, columns with V[i] == 0, columns in which s == 0 while some W entry of the window is
    not) over the batch, on the tables as they come in"""
    u, i = np.asarray(users, np.int64), np.asarray(items, np.int64)
    rec = np.asarray(recents, np.int64).reshape(len(u), -1)
    s = context(W, rec)
    cancelled = (s == 0) & (W[rec] != 0).any(axis=1)
    return int((P[u] == 0).sum()), int((V[i] == 0).sum()), int(cancelled.sum())


def gradients(P, V, W, users, recents, items, labels, loss, reg):
    """(loss, G_P, G_V, G_W) of one batch in the dtype of P: NPE.py:54-71 and its derivative"""
    dt = P.dtype.type
    u, i = np.asarray(users, np.int64), np.asarray(items, np.int64)
    rec = np.asarray(recents, np.int64).reshape(len(u), -1)
    N, L = rec.shape
    p, v, rows = P[u], V[i], W[rec]
    s = context(W, rec)
    q, rv = relu(p) + relu(s), relu(v)
    x = (rv * q).sum(axis=1)
    y = np.asarray(labels, P.dtype)
    if loss == "square":
        total, g = ((y - x) ** 2).sum(), dt(-2) * (y - x)
    else:
        total = (np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).mean() if N else dt(0)
        g = (dt(1) / (dt(1) + np.exp(-x)) - y) / dt(max(N, 1))
    total = total + dt(reg) * dt(0.5) * ((p ** 2).sum() + (v ** 2).sum() + (rows ** 2).sum())   # per occurrence
    GP, GV, GW = np.zeros_like(P), np.zeros_like(V), np.zeros_like(W)
    grv = g[:, None] * rv
    np.add.at(GP, u, grv * gate(p) + dt(reg) * p)
    np.add.at(GV, i, g[:, None] * q * gate(v) + dt(reg) * v)
    ds = grv * gate(s)
    np.add.at(GW, rec.reshape(-1), (ds[:, None, :] + dt(reg) * rows).reshape(N * L, -1))
    return total, GP, GV, GW


def step(st, users, recents, items, labels, loss, reg):
    """one sess.run((loss, optimizer)): returns the pre-update loss"""
    total, GP, GV, GW = gradients(st.var["P"], st.var["V"], st.var["W"], users, recents, items, labels, loss, reg)
    st.apply("P", GP, np.unique(np.asarray(users, np.int64)))
    st.apply("V", GV, np.unique(np.asarray(items, np.int64)))
    st.apply("W", GW, np.unique(np.asarray(recents, np.int64).reshape(-1)))
    st.b1p, st.b2p = st.b1p * 0.9, st.b2p * 0.999
    return float(total)


# ------------------------------------------------------------------ predict
def user_factors(P, W, users, last):
    """h_u [n, d] = relu(P[u]) + relu(the sum of W over the user's valid last items); none (deviation a): relu(P[u])
    alone.  At L = 1 (deviation b) the context is the one last item, as in training."""
    P, W = np.asarray(P, np.float64), np.asarray(W, np.float64)
    out = np.empty((len(users), P.shape[1]))
    for k, u in enumerate(users):
        tail = np.asarray([int(r) for r in last[u] if r >= 0], np.int64)
        out[k] = relu(P[u]) + relu(context(W, tail[None])[0])
    return out


def predict(P, V, W, users, last):
    """NPE.py:114-142: every item against h_u"""
    return user_factors(P, W, users, last) @ relu(np.asarray(V, np.float64)).T


def edge_patterns(users, recents, items):
    """the duplicate patterns a golden batch holds: a user twice; an item that is the target of one instance and a
    recent of another; an item twice among one window's recents"""
    users, items = np.asarray(users).tolist(), np.asarray(items).tolist()
    rec = np.asarray(recents).reshape(len(users), -1)
    return {"user twice": len(set(users)) < len(users),
            "recent and target": bool(set(rec.reshape(-1).tolist()) & set(items)),
            "item twice in a window": any(len(set(r)) < len(r) for r in rec.tolist())}
