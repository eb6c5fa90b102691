"""A float64 numpy restatement of Fossil (model/sequential_recommender/Fossil.py:59-102, util/learner.py, TF-1.12's
optimiser kernels) for the Fossil tests: the instance rule, one training step for every loss and learner (dense
application for c1 and eta_bias, row application for Q, bias and eta) and predict().  Checked against the reference
class's own f64 trace in test_fossil_cpu.py; the GPU tests use it for the shapes the trace does not hold.

An instance is (user u, item i, excluded item e or none, count n, recents r_0..r_{L-1} most recent first):
    p = sum_{h in R_u \\ {e}} c1[h]    w_l = eta_bias[l] + eta[u, l]    s = sum_l w_l c1[r_l]
    out = n^-alpha <p, Q[i]> + <s, Q[i]> + bias[i]
"""
import numpy as np

import fism_restatement as F
from fism_restatement import golden_matrix, history          # noqa: F401

TABLES = ("c1", "Q", "bias", "eta", "eta_bias")
# case -> (loss, learner, pairwise, high_order, regs, alpha)
CASES = {
    "bpr_adagrad": ("bpr", "adagrad", True, 3, (0.0, 0.0, 0.0), 0.5),         # conf/Fossil.properties
    "bpr_adam": ("bpr", "adam", True, 3, (0.01, 0.02, 0.005), 0.5),
    "hinge_adam": ("hinge", "adam", True, 3, (0.01, 0.02, 0.005), 0.5),
    "ce_adam": ("cross_entropy", "adam", False, 3, (0.01, 0.02, 0.005), 0.5),
    "square_gd": ("square", "gd", False, 3, (0.01, 0.02, 0.005), 0.5),
    "square_rmsprop": ("square", "rmsprop", False, 3, (0.01, 0.02, 0.005), 0.5),
    "square_momentum": ("square", "momentum", False, 3, (0.01, 0.02, 0.005), 0.5),
    "l1_square_adam": ("square", "adam", False, 1, (0.01, 0.02, 0.005), 0.5),
    "l2_bpr_adam": ("bpr", "adam", True, 2, (0.01, 0.02, 0.005), 0.5),
    "alpha0_ce_adam": ("cross_entropy", "adam", False, 3, (0.03, 0.02, 0.04), 0.0),
}


class State(F.State):
    """the optimiser state of fism_restatement on Fossil's five tables"""

    def __init__(self, c1, Q, bias, eta, eta_bias, learner="adam", lr=0.01, momentum=0.9):
        f = lambda x: np.array(x, dtype=np.float64)
        self.var = {"c1": f(c1), "Q": f(Q), "bias": f(np.zeros(len(Q)) if bias is None else bias), "eta": f(eta),
                    "eta_bias": f(eta_bias).reshape(-1)}
        self.learner, self.lr, self.momentum = learner, lr, momentum
        init = {"adam": 0.0, "gd": 0.0, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        self.s0 = {k: np.full_like(v, init) for k, v in self.var.items()}
        self.s1 = {k: np.zeros_like(v) for k, v in self.var.items()}
        self.b1p, self.b2p = 0.9, 0.999


def initial_tables(g, case):
    """(c1, Q, bias, eta, eta_bias) every case starts from: eta and eta_bias are the first L columns of the stored ones"""
    L = CASES[case][3]
    return [g["c1_0"], g["Q_0"], g["bias_0"], np.ascontiguousarray(g["eta_0"][:, :L]), g["eta_bias_0"][:L].copy()]


def golden_tables(g, case, tag, step):
    """(c1, Q, bias, eta, eta_bias) of the trace after `step` (0-based), full size, in the trace's width"""
    dt = np.float32 if tag == "f32" else np.float64
    out = []
    for name, init in zip(TABLES, initial_tables(g, case)):
        t = init.astype(np.float64)
        rows = g["%s_rows_%s" % (case, name)]
        t[rows] = t[rows] + g["%s_%s_%s" % (case, tag, name)][step]
        out.append(t.astype(dt))
    return out


def sequences(g):
    """{user: [items by time]} of the golden's train pattern"""
    ptr, seq = g["seq_ptr"], g["seq"]
    return {u: seq[ptr[u]:ptr[u + 1]].tolist() for u in range(len(ptr) - 1) if ptr[u + 1] > ptr[u]}


def takes_part(R, L, u, recents, items, n_users=None):
    """the slot rule: user and items table rows, |R_u| > L, every recent a train item of the user"""
    U, I = R.shape
    if not 0 <= u < U or any(not 0 <= i < I for i in items):
        return False
    row = R.indices[R.indptr[u]:R.indptr[u + 1]]
    return len(row) > L and all(r in row for r in recents)


def instances(R, L, users, recents, items, third, pairwise):
    """[(slot, user, item, excluded or -1, n, once?)]: pointwise one per slot; pairwise the positive sides, then the
    negative sides.  once: the instance carries the terms that enter once per pointwise instance / per pair"""
    deg = np.diff(R.indptr)
    rec = np.asarray(recents).reshape(len(users), L)
    if not pairwise:
        keep = [k for k in range(len(users)) if takes_part(R, L, int(users[k]), rec[k], [int(items[k])])]
        return [(k, int(users[k]), int(items[k]), int(items[k]) if third[k] > 0.5 else -1,
                 int(deg[users[k]]) - 1 if third[k] > 0.5 else int(deg[users[k]]), True) for k in keep]
    keep = [k for k in range(len(users))
            if takes_part(R, L, int(users[k]), rec[k], [int(items[k]), int(third[k])])]
    return [(k, int(users[k]), int(items[k]), int(items[k]), int(deg[users[k]]) - 1, True) for k in keep] + \
           [(k, int(users[k]), int(third[k]), -1, int(deg[users[k]]), False) for k in keep]


def step(st, R, users, recents, items, third, pairwise, loss, alpha, regs):
    """one sess.run((loss, optimizer)): returns the pre-update loss.  recents [B, L], most recent first"""
    c1, Q, bias, eta, eb = (st.var[k] for k in TABLES)
    L, d = eta.shape[1], c1.shape[1]
    B = len(users)
    rec_all = np.asarray(recents, np.int64).reshape(B, L)
    inst = instances(R, L, users, recents, items, third, pairwise)
    N = len(inst)
    slot = np.asarray([k for k, *_ in inst], np.int64)
    us = np.asarray([u for _, u, *_ in inst], np.int64)
    it = np.asarray([i for _, _, i, *_ in inst], np.int64)
    p = np.stack([c1[history(R, u, e)].sum(axis=0) for _, u, _, e, _, _ in inst]) if N else np.zeros((0, d))
    coeff = np.asarray([float(n) ** -alpha for *_, n, _ in inst])
    once = np.asarray([1.0 if o else 0.0 for *_, o in inst])
    rec = rec_all[slot]                                                   # [N, L]
    w = eb[None, :] + eta[us]                                             # [N, L]
    short = c1[rec]                                                       # [N, L, d]
    s = (w[:, :, None] * short).sum(axis=1)
    out = coeff * (p * Q[it]).sum(axis=1) + (s * Q[it]).sum(axis=1) + bias[it]
    if not pairwise:
        y = np.asarray(third, np.float64)[slot]
        if loss == "square":
            total, dout = ((y - out) ** 2).sum(), -2.0 * (y - out)
        else:
            # the mean runs over the batch as fed: slots that take no part are not in the reference's feed at all, and
            # the engine divides by the batch's length — the tests that drop slots use `square`
            total = (np.maximum(out, 0) - out * y + np.log1p(np.exp(-np.abs(out)))).sum() / max(B, 1)
            dout = (1.0 / (1.0 + np.exp(-out)) - y) / max(B, 1)
    else:
        h = N // 2
        yy = out[:h] - out[h:]
        if loss == "bpr":
            total, dl = np.logaddexp(0.0, -yy).sum(), -1.0 / (1.0 + np.exp(yy))
        elif loss == "hinge":
            total, dl = np.maximum(yy + 1, 0).sum(), (yy + 1 > 0).astype(np.float64)
        else:
            total, dl = ((1 - yy) ** 2).sum(), -2.0 * (1 - yy)
        dout = np.concatenate([dl, -dl])
    total += regs[0] * 0.5 * (once[:, None] * p * p).sum() + regs[1] * 0.5 * (Q[it] ** 2).sum() \
        + regs[1] * 0.5 * (once[:, None, None] * short ** 2).sum() \
        + regs[2] * 0.5 * ((once[:, None] * eta[us] ** 2).sum() + (eb ** 2).sum())
    g = (dout * coeff)[:, None] * Q[it] + regs[0] * once[:, None] * p
    G = {k: np.zeros_like(st.var[k]) for k in TABLES}
    for b, (_, u, _, e, _, _) in enumerate(inst):
        G["c1"][history(R, u, e)] += g[b]
    g_short = (dout[:, None] * w)[:, :, None] * Q[it][:, None, :] + regs[1] * once[:, None, None] * short
    np.add.at(G["c1"], rec.reshape(-1), g_short.reshape(-1, d))
    np.add.at(G["Q"], it, dout[:, None] * (coeff[:, None] * p + s) + regs[1] * Q[it])
    np.add.at(G["bias"], it, dout)
    dots = (short * Q[it][:, None, :]).sum(axis=2)                        # [N, L]
    g_w = dout[:, None] * dots
    np.add.at(G["eta"], us, g_w + regs[2] * once[:, None] * eta[us])
    G["eta_bias"] = g_w.sum(axis=0) + regs[2] * eb
    st.apply("c1", G["c1"], None)
    st.apply("eta_bias", G["eta_bias"], None)
    st.apply("Q", G["Q"], np.unique(it))
    st.apply("bias", G["bias"], np.unique(it))
    st.apply("eta", G["eta"], np.unique(us))
    st.b1p, st.b2p = st.b1p * 0.9, st.b2p * 0.999
    return total


def last_items(seqs, n_users, L):
    """deviations 2 and 3: the last min(L, |R_u|) items ascending in time from eta column 0, -1 in the other columns"""
    last = np.full((n_users, L), -1, np.int32)
    for u, s in seqs.items():
        tail = s[max(len(s) - L, 0):]
        last[u, :len(tail)] = tail
    return last


def predict(R, c1, Q, bias, eta, eta_bias, users, alpha, last):
    """Fossil.py:177-217: the whole train row, n = |R_u|, the last items at the eta columns `last` names"""
    c1, Q, bias, eta, eb = (np.asarray(x, np.float64) for x in (c1, Q, bias, eta, eta_bias))
    eb = eb.reshape(-1)
    out = np.empty((len(users), Q.shape[0]))
    for k, u in enumerate(users):
        row = R.indices[R.indptr[u]:R.indptr[u + 1]]
        f = float(len(row)) ** -alpha * c1[row].sum(axis=0) if len(row) else np.zeros(c1.shape[1])
        for l, r in enumerate(last[u]):
            if r >= 0:
                f = f + (eb[l] + eta[u, l]) * c1[r]
        out[k] = Q @ f + bias
    return out


def edge_patterns(users, recents, items, third, pairwise):
    """which duplicate patterns a batch holds: a user twice; an item twice as target; an item that is a recent here
    and a target there; one item at two different eta columns of two instances of one user"""
    users, items = np.asarray(users).tolist(), np.asarray(items).tolist()
    rec = np.asarray(recents).reshape(len(users), -1)
    targets = items + (np.asarray(third).tolist() if pairwise else [])
    cols = {}
    for u, r in zip(users, rec):
        for l, h in enumerate(r.tolist()):
            cols.setdefault((u, h), set()).add(l)
    return {"user twice": len(set(users)) < len(users), "target twice": len(set(targets)) < len(targets),
            "recent and target": bool(set(rec.reshape(-1).tolist()) & set(targets)),
            "two columns": rec.shape[1] == 1 or any(len(v) > 1 for v in cols.values())}
