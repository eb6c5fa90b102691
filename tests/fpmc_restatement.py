"""A float64 numpy restatement of FPMC (model/sequential_recommender/FPMC.py:61-88, util/learner.py, TF-1.12's sparse
optimiser kernels) for the FPMC tests: one training step for every loss and learner, predict(), and the duplicate
patterns the golden batches hold.  Checked against the reference class's own f64 trace in test_fpmc_cpu.py; the GPU
tests use it for the shapes the trace does not hold."""
import numpy as np

import fism_restatement as F

TABLES = ("UI", "IU", "IL", "LI")
CASES = {"ce_adam": ("cross_entropy", "adam", False), "square_adam": ("square", "adam", False),
         "square_gd": ("square", "gd", False), "square_adagrad": ("square", "adagrad", False),
         "square_rmsprop": ("square", "rmsprop", False), "square_momentum": ("square", "momentum", False),
         "bpr_adam": ("bpr", "adam", True)}


class State(F.State):
    """the optimiser state of fism_restatement on FPMC's four tables; every one gets the sparse application"""

    def __init__(self, UI, IU, IL, LI, learner="adam", lr=0.01, momentum=0.9):
        f = lambda x: np.array(x, dtype=np.float64)
        self.var = {"UI": f(UI), "IU": f(IU), "IL": f(IL), "LI": f(LI)}
        self.learner, self.lr, self.momentum = learner, lr, momentum
        init = {"adam": 0.0, "gd": 0.0, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        self.s0 = {k: np.full_like(v, init) for k, v in self.var.items()}
        self.s1 = {k: np.zeros_like(v) for k, v in self.var.items()}
        self.b1p, self.b2p = 0.9, 0.999


def golden_tables(g, case, tag, step):
    """(UI, IU, IL, LI) of the trace after `step` (0-based), full size, in the trace's width"""
    dt = np.float32 if tag == "f32" else np.float64
    out = []
    for name in TABLES:
        t = g[name + "_0"].astype(np.float64)
        rows = g["%s_rows_%s" % (case, name)]
        t[rows] = t[rows] + g["%s_%s_%s" % (case, tag, name)][step]
        out.append(t.astype(dt))
    return out


def sequences(g):
    """{user: [items by time]} of the golden's train pattern"""
    ptr, seq = g["seq_ptr"], g["seq"]
    return {u: seq[ptr[u]:ptr[u + 1]].tolist() for u in range(len(ptr) - 1) if ptr[u + 1] > ptr[u]}


def scores(UI, IU, IL, LI, u, l, i):
    """x(u, l, i) = <UI_u, IU_i> + <IL_i, LI_l>  (FPMC.py:64-69)"""
    return (UI[u] * IU[i]).sum(axis=1) + (IL[i] * LI[l]).sum(axis=1)


def step(st, users, recent, items, third, pairwise, loss, reg):
    """one sess.run((loss, optimizer)): returns the pre-update loss"""
    UI, IU, IL, LI = (st.var[k] for k in TABLES)
    u, l, i = (np.asarray(x, np.int64) for x in (users, recent, items))
    N = len(u)
    x = scores(UI, IU, IL, LI, u, l, i)
    sq = (UI[u] ** 2).sum() + (IU[i] ** 2).sum() + (IL[i] ** 2).sum() + (LI[l] ** 2).sum()
    if not pairwise:
        y = np.asarray(third, np.float64)
        if loss == "square":
            total, g = ((y - x) ** 2).sum(), -2.0 * (y - x)
        else:
            total = (np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).mean() if N else 0.0
            g = (1.0 / (1.0 + np.exp(-x)) - y) / max(N, 1)
    else:
        j = np.asarray(third, np.int64)
        yy = x - scores(UI, IU, IL, LI, u, l, j)
        if loss == "bpr":
            total, g = np.logaddexp(0.0, -yy).sum(), -1.0 / (1.0 + np.exp(yy))
        elif loss == "hinge":
            total, g = np.maximum(yy + 1, 0).sum(), (yy + 1 > 0).astype(np.float64)
        else:
            total, g = ((1 - yy) ** 2).sum(), -2.0 * (1 - yy)
        sq += (IU[j] ** 2).sum() + (IL[j] ** 2).sum()
    total += reg * 0.5 * sq
    G = {k: np.zeros_like(st.var[k]) for k in TABLES}
    gc = g[:, None]
    np.add.at(G["UI"], u, gc * IU[i] + reg * UI[u])
    np.add.at(G["LI"], l, gc * IL[i] + reg * LI[l])
    np.add.at(G["IU"], i, gc * UI[u] + reg * IU[i])
    np.add.at(G["IL"], i, gc * LI[l] + reg * IL[i])
    item_rows = i
    if pairwise:
        np.add.at(G["UI"], u, -gc * IU[j])
        np.add.at(G["LI"], l, -gc * IL[j])
        np.add.at(G["IU"], j, -gc * UI[u] + reg * IU[j])
        np.add.at(G["IL"], j, -gc * LI[l] + reg * IL[j])
        item_rows = np.concatenate([i, j])
    for k, rows in (("UI", u), ("IU", item_rows), ("IL", item_rows), ("LI", l)):
        st.apply(k, G[k], np.unique(rows))
    st.b1p, st.b2p = st.b1p * 0.9, st.b2p * 0.999
    return total


def predict(UI, IU, IL, LI, users, last):
    """FPMC.py:140-152: every item against the user's most recent train item; last < 0 (no train items): <UI_u, IU_i>"""
    UI, IU, IL, LI = (np.asarray(x, np.float64) for x in (UI, IU, IL, LI))
    out = np.empty((len(users), IU.shape[0]))
    for k, u in enumerate(users):
        out[k] = IU @ UI[u] + (IL @ LI[last[u]] if last[u] >= 0 else 0.0)
    return out


def last_items(seqs, n_users):
    last = np.full(n_users, -1, np.int32)
    for u, s in seqs.items():
        last[u] = s[-1]
    return last


def edge_patterns(users, recent, items, third, pairwise):
    """which of the five duplicate patterns a batch holds: a user twice; an item twice as target; an item twice as
    recent; an item that is recent here and target there; an item that is positive here and negative there (pairwise)
    or carries label 1 here and label 0 there (pointwise)"""
    users, recent, items = (np.asarray(x).tolist() for x in (users, recent, items))
    twice = lambda xs: len(set(xs)) < len(xs)
    if pairwise:
        negs = np.asarray(third).tolist()
        targets = items + negs
        both = set(items) & set(negs)
    else:
        y = np.asarray(third)
        targets = items
        both = {i for i, t in zip(items, y) if t > 0.5} & {i for i, t in zip(items, y) if t <= 0.5}
    return {"user twice": twice(users), "target twice": twice(items), "recent twice": twice(recent),
            "recent and target": bool(set(recent) & set(targets)), "both signs": bool(both)}
