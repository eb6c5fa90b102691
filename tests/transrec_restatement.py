"""A float64 numpy restatement of TransRec (model/sequential_recommender/TransRec.py:66-107, util/learner.py, TF-1.12's
optimiser kernels) for the TransRec tests: the gradients of one batch by hand, one training step for every loss and
learner (sparse application for P / Q / b, dense for T), predict(), and the duplicate patterns the golden batches hold.
Checked against the reference class's own f64 trace in test_transrec_cpu.py; the GPU tests use it for the shapes the
trace does not hold."""
import numpy as np

import fism_restatement as F
from fpmc_restatement import last_items, sequences          # noqa: F401

TABLES = ("P", "Q", "b", "T")
ROWS = ("P", "Q", "b")
REG = 0.01
# case -> (loss, learner, pairwise, reg_mf)
CASES = {"ce_adam": ("cross_entropy", "adam", False, REG), "square_adam": ("square", "adam", False, REG),
         "square_gd": ("square", "gd", False, REG), "square_adagrad": ("square", "adagrad", False, REG),
         "square_rmsprop": ("square", "rmsprop", False, REG), "square_momentum": ("square", "momentum", False, REG),
         "bpr_adam": ("bpr", "adam", True, REG), "hinge_adam": ("hinge", "adam", True, REG),
         "bpr_adam_reg0": ("bpr", "adam", True, 0.0)}
PREDICT_CASE = "ce_adam"


class State(F.State):
    """the optimiser state of fism_restatement on TransRec's four tables; b and T as vectors"""

    def __init__(self, P, Q, b, T, learner="adam", lr=0.01, momentum=0.9):
        f = lambda x: np.array(x, dtype=np.float64)
        self.var = {"P": f(P), "Q": f(Q), "b": f(b).reshape(-1), "T": f(T).reshape(-1)}
        self.learner, self.lr, self.momentum = learner, lr, momentum
        init = {"adam": 0.0, "gd": 0.0, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        self.s0 = {k: np.full_like(v, init) for k, v in self.var.items()}
        self.s1 = {k: np.zeros_like(v) for k, v in self.var.items()}
        self.b1p, self.b2p = 0.9, 0.999

    def tables(self):
        return [self.var[k] for k in TABLES]


def golden_tables(g, case, tag, step):
    """(P, Q, b, T) of the trace after `step` (0-based; -1: the initial ones), full size, in the trace's width; b and T
    as vectors"""
    dt = np.float32 if tag == "f32" else np.float64
    out = []
    for name in TABLES:
        t = g[name + "_0"].astype(np.float64)
        if step >= 0:
            if name == "T":
                t = t + g["%s_%s_T" % (case, tag)][step]
            else:
                rows = g["%s_rows_%s" % (case, name)]
                t[rows] = t[rows] + g["%s_%s_%s" % (case, tag, name)][step]
        out.append(t.astype(dt).reshape(-1) if name in ("b", "T") else t.astype(dt))
    return out


def translation(P, Q, T, u, l, i):
    """v = P_u + T + Q_l - Q_i  (TransRec.py:75-76)"""
    return P[u] + T[None, :] + Q[l] - Q[i]


def gradients(P, Q, b, T, users, recent, items, third, pairwise, loss, reg):
    """(loss, {table: gradient}) of one batch: TransRec.py:77-91 and its derivative by hand.  The training score is
    b_i - |v|^2, the SQUARED distance; T enters the regulariser once per step; the second inference's lookups of P_u
    and Q_l carry no regulariser term"""
    u, l, i = (np.asarray(x, np.int64) for x in (users, recent, items))
    N = len(u)
    v = translation(P, Q, T, u, l, i)
    x = b[i] - (v * v).sum(axis=1)
    sq = (P[u] ** 2).sum() + (Q[l] ** 2).sum() + (Q[i] ** 2).sum() + (b[i] ** 2).sum() + (T ** 2).sum()
    if not pairwise:
        y = np.asarray(third, np.float64)
        if loss == "square":
            total, g = ((y - x) ** 2).sum(), -2.0 * (y - x)
        else:
            total = (np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).mean() if N else 0.0
            g = (1.0 / (1.0 + np.exp(-x)) - y) / max(N, 1)
    else:
        j = np.asarray(third, np.int64)
        v2 = translation(P, Q, T, u, l, j)
        yy = x - (b[j] - (v2 * v2).sum(axis=1))
        if loss == "bpr":
            total, g = np.logaddexp(0.0, -yy).sum(), -1.0 / (1.0 + np.exp(yy))
        elif loss == "hinge":
            total, g = np.maximum(yy + 1, 0).sum(), (yy + 1 > 0).astype(np.float64)
        else:
            total, g = ((1 - yy) ** 2).sum(), -2.0 * (1 - yy)
        sq += (Q[j] ** 2).sum() + (b[j] ** 2).sum()
    total += reg * 0.5 * sq
    G = {"P": np.zeros_like(P), "Q": np.zeros_like(Q), "b": np.zeros_like(b), "T": reg * T}
    gc = g[:, None]
    np.add.at(G["P"], u, -2.0 * gc * v + reg * P[u])
    np.add.at(G["Q"], l, -2.0 * gc * v + reg * Q[l])
    np.add.at(G["Q"], i, 2.0 * gc * v + reg * Q[i])
    np.add.at(G["b"], i, g + reg * b[i])
    G["T"] = G["T"] + (-2.0 * gc * v).sum(axis=0)
    if pairwise:
        np.add.at(G["P"], u, 2.0 * gc * v2)
        np.add.at(G["Q"], l, 2.0 * gc * v2)
        np.add.at(G["Q"], j, -2.0 * gc * v2 + reg * Q[j])
        np.add.at(G["b"], j, -g + reg * b[j])
        G["T"] = G["T"] + (2.0 * gc * v2).sum(axis=0)
    return total, G


def touched(users, recent, items, third, pairwise):
    """{table: the rows the batch looks up}: P by the users, Q in all three roles, b by targets and negatives"""
    u, l, i = (np.asarray(x, np.int64) for x in (users, recent, items))
    tj = [np.asarray(third, np.int64)] if pairwise else []
    return {"P": np.unique(u), "Q": np.unique(np.concatenate([l, i] + tj)), "b": np.unique(np.concatenate([i] + tj))}


def step(st, users, recent, items, third, pairwise, loss, reg):
    """one sess.run((loss, optimizer)): returns the pre-update loss"""
    total, G = gradients(*st.tables(), users, recent, items, third, pairwise, loss, reg)
    for k, rows in touched(users, recent, items, third, pairwise).items():
        st.apply(k, G[k], rows)
    st.apply("T", G["T"], None)
    st.b1p, st.b2p = st.b1p * 0.9, st.b2p * 0.999
    return float(total)


def predict(P, Q, b, T, users, last):
    """TransRec.py:102-107, 153-161: b_j - |P_u + T + Q_last(u) - Q_j|, the distance NOT squared; last < 0 (no train
    items): the query is P_u + T"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    b, T = np.asarray(b, np.float64).reshape(-1), np.asarray(T, np.float64).reshape(-1)
    out = np.empty((len(users), Q.shape[0]))
    for k, u in enumerate(users):
        q = P[u] + T + (Q[last[u]] if last[u] >= 0 else 0.0)
        out[k] = b - np.sqrt(((q[None, :] - Q) ** 2).sum(axis=1))
    return out


def edge_patterns(users, recent, items, third, pairwise):
    """the duplicate patterns a golden batch holds: a user twice; an item that is a recent here and a target there (and,
    pairwise, a negative elsewhere); an instance whose target is its own recent item"""
    users, recent, items = (np.asarray(x).tolist() for x in (users, recent, items))
    both = set(recent) & set(items)
    out = {"user twice": len(set(users)) < len(users), "recent and target": bool(both),
           "target is the recent": any(l == i for l, i in zip(recent, items))}
    if pairwise:
        out["recent, target and negative"] = bool(both & set(np.asarray(third).tolist()))
    return out
