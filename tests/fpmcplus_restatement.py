"""A numpy restatement of FPMCplus (model/sequential_recommender/FPMCplus.py:73-119, util/learner.py, TF-1.12's
optimiser kernels) for the FPMCplus tests: forward, hand gradients for all seven tables, one training step for every
loss and learner (sparse application for UI / IU / IL / LI, dense for W / b / h), and predict() with the stated
deviations: a recent < 0 is a slot that takes no part in the softmax or in any gradient; none present: x = <UI_u, IU_i>.
Checked against the reference class's own f64 trace and against torch.autograd in test_fpmcplus_cpu.py; the GPU tests
use it for the shapes the trace does not hold.  `gradients` computes in the dtype of the tables it is given, so that
a long run can be restated in float32 as well."""
import numpy as np

import fism_restatement as F
from fpmc_restatement import sequences          # noqa: F401

TABLES = ("UI", "IU", "IL", "LI", "W", "b", "h")
ROWS = ("UI", "IU", "IL", "LI")
# case -> (loss, learner, pairwise, high_order)
CASES = {"bpr_adam": ("bpr", "adam", True, 3), "hinge_gd": ("hinge", "gd", True, 2),
         "square_rmsprop": ("square", "rmsprop", True, 5), "ce_adagrad": ("cross_entropy", "adagrad", False, 3),
         "square_momentum": ("square", "momentum", False, 2)}
PREDICT_CASE = "bpr_adam"


class State(F.State):
    """the optimiser state of fism_restatement on the seven tables, in the dtype asked for"""

    def __init__(self, UI, IU, IL, LI, W, b, h, learner="adam", lr=0.01, momentum=0.9, dtype=np.float64):
        f = lambda x: np.array(x, dtype=dtype)
        self.var = {"UI": f(UI), "IU": f(IU), "IL": f(IL), "LI": f(LI), "W": f(W),
                    "b": f(b).reshape(-1), "h": f(h).reshape(-1)}
        self.learner, self.lr, self.momentum = learner, dtype(lr), dtype(momentum)
        init = {"adam": 0.0, "gd": 0.0, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        self.s0 = {k: np.full_like(v, init) for k, v in self.var.items()}
        self.s1 = {k: np.zeros_like(v) for k, v in self.var.items()}
        self.b1p, self.b2p = dtype(0.9), dtype(0.999)

    def tables(self):
        return [self.var[k] for k in TABLES]


def golden_tables(g, case, tag, step):
    """the seven tables of the trace after `step` (0-based; -1: the initial ones), full size, in the trace's width;
    b and h as vectors"""
    dt = np.float32 if tag == "f32" else np.float64
    out = []
    for name in TABLES:
        t = g["%s_%s_0" % (case, name) if name == "h" else name + "_0"].astype(np.float64)
        if step >= 0:
            if name in ROWS:
                rows = g["%s_rows_%s" % (case, name)]
                t[rows] = t[rows] + g["%s_%s_%s" % (case, tag, name)][step]
            else:
                t = t + g["%s_%s_%s" % (case, tag, name)][step]
        out.append(t.astype(dt).reshape(-1) if name in ("b", "h") else t.astype(dt))
    return out


# ------------------------------------------------------------------ forward
def attention(UI, IL, LI, W, b, h, u, i, rec):
    """(a [N, L, w], alpha [N, L], s [N, d], present [N, L]) of FPMCplus.py:73-93 for targets i"""
    d = UI.shape[1]
    present = rec >= 0
    rows = LI[np.where(present, rec, 0)] * present[:, :, None].astype(UI.dtype)
    pre = (UI[u] @ W[:d])[:, None, :] + (IL[i] @ W[d:2 * d])[:, None, :] + rows @ W[2 * d:] + b[None, None, :]
    a = np.tanh(pre)
    ex = np.exp(a @ h) * present.astype(UI.dtype)
    tot = ex.sum(axis=1, keepdims=True)
    alpha = np.divide(ex, tot, out=np.zeros_like(ex), where=tot > 0)
    s = (alpha[:, :, None] * rows).sum(axis=1)
    return a, alpha, s, present, rows


def scores(UI, IU, IL, LI, W, b, h, u, i, rec):
    """x(u, i) of FPMCplus.py:95-106"""
    _, _, s, _, _ = attention(UI, IL, LI, W, b, h, u, i, rec)
    return (UI[u] * IU[i]).sum(axis=1) + (IL[i] * s).sum(axis=1)


def loss_and_g(x, xn, third, pairwise, loss, dt):
    N = len(x)
    if not pairwise:
        y = np.asarray(third, x.dtype)
        if loss == "square":
            return ((y - x) ** 2).sum(), dt(-2) * (y - x)
        total = (np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).mean() if N else dt(0)
        return total, (dt(1) / (dt(1) + np.exp(-x)) - y) / dt(max(N, 1))
    yy = x - xn
    if loss == "bpr":
        return np.logaddexp(dt(0), -yy).sum(), dt(-1) / (dt(1) + np.exp(yy))
    if loss == "hinge":
        return np.maximum(yy + 1, 0).sum(), (yy + 1 > 0).astype(x.dtype)
    return ((1 - yy) ** 2).sum(), dt(-2) * (1 - yy)


def gradients(UI, IU, IL, LI, W, b, h, users, recents, items, third, pairwise, loss, reg_mf, reg_w):
    """(loss, {table: gradient}) of one batch in the dtype of UI: FPMCplus.py:108-119 and its derivative by hand"""
    dt = UI.dtype.type
    d = UI.shape[1]
    u, i = np.asarray(users, np.int64), np.asarray(items, np.int64)
    rec = np.asarray(recents, np.int64).reshape(len(u), -1)
    N, L = rec.shape
    sides = [i] + ([np.asarray(third, np.int64)] if pairwise else [])
    fwd = [attention(UI, IL, LI, W, b, h, u, it, rec) for it in sides]
    xs = [(UI[u] * IU[it]).sum(axis=1) + (IL[it] * f[2]).sum(axis=1) for it, f in zip(sides, fwd)]
    total, g = loss_and_g(xs[0], xs[1] if pairwise else None, third, pairwise, loss, dt)
    present, rows = fwd[0][3], fwd[0][4]
    sq = (UI[u] ** 2).sum() + (rows ** 2).sum() + sum((IU[it] ** 2).sum() + (IL[it] ** 2).sum() for it in sides)
    total = total + dt(reg_mf) * dt(0.5) * sq
    if pairwise:
        total = total + dt(reg_w) * dt(0.5) * ((W ** 2).sum() + (h ** 2).sum())
    G = {k: np.zeros_like(t) for k, t in zip(TABLES, (UI, IU, IL, LI, W, b, h))}
    np.add.at(G["UI"], u, dt(reg_mf) * UI[u])
    flat = np.where(present, rec, 0).reshape(-1)
    np.add.at(G["LI"], flat, (dt(reg_mf) * rows).reshape(N * L, d))
    for side, (it, (a, alpha, s, _, _)) in enumerate(zip(sides, fwd)):
        gs = (g if side == 0 else -g)[:, None]
        e = (IL[it][:, None, :] * rows).sum(axis=2)                        # <IL_i, LI_{r_l}>
        dA = gs * alpha * (e - (IL[it] * s).sum(axis=1)[:, None])
        delta = dA[:, :, None] * h[None, None, :] * (1 - a * a)            # [N, L, w]
        Delta = delta.sum(axis=1)
        np.add.at(G["IU"], it, gs * UI[u] + dt(reg_mf) * IU[it])
        np.add.at(G["UI"], u, gs * IU[it] + Delta @ W[:d].T)
        np.add.at(G["IL"], it, gs * s + Delta @ W[d:2 * d].T + dt(reg_mf) * IL[it])
        gl = (gs * alpha)[:, :, None] * IL[it][:, None, :] + delta @ W[2 * d:].T
        np.add.at(G["LI"], flat, (gl * present[:, :, None].astype(UI.dtype)).reshape(N * L, d))
        G["W"][:d] += UI[u].T @ Delta
        G["W"][d:2 * d] += IL[it].T @ Delta
        G["W"][2 * d:] += rows.reshape(N * L, d).T @ delta.reshape(N * L, -1)
        G["b"] += Delta.sum(axis=0)
        G["h"] += (dA[:, :, None] * a).sum(axis=(0, 1))
    if pairwise:
        G["W"] += dt(reg_w) * W
        G["h"] += dt(reg_w) * h
    return total, G


def step(st, users, recents, items, third, pairwise, loss, reg_mf, reg_w):
    """one sess.run((loss, optimizer)): returns the pre-update loss"""
    total, G = gradients(*st.tables(), users, recents, items, third, pairwise, loss, reg_mf, reg_w)
    u, i = np.asarray(users, np.int64), np.asarray(items, np.int64)
    rec = np.asarray(recents, np.int64).reshape(-1)
    item_rows = np.concatenate([i, np.asarray(third, np.int64)]) if pairwise else i
    for k, rows in (("UI", u), ("IU", item_rows), ("IL", item_rows), ("LI", rec[rec >= 0])):
        st.apply(k, G[k], np.unique(rows))
    for k in ("W", "b", "h"):
        st.apply(k, G[k], None)
    st.b1p, st.b2p = st.b1p * st.b1p.dtype.type(0.9), st.b2p * st.b2p.dtype.type(0.999)
    return float(total)


# ------------------------------------------------------------------ predict
def last_items_table(seqs, n_users, L):
    """[n_users, L]: the user's last min(|R_u|, L) items by time, oldest first, padded with -1"""
    out = np.full((n_users, L), -1, np.int32)
    for u, s in seqs.items():
        tail = list(s)[-L:]
        out[u, :len(tail)] = tail
    return out


def predict(UI, IU, IL, LI, W, b, h, users, last):
    """FPMCplus.py:177-191 in float64: every item against the user's last items; deviations (a) and (b): the softmax
    covers the present slots alone, none present scores <UI_u, IU_i>"""
    UI, IU, IL, LI, W = (np.asarray(x, np.float64) for x in (UI, IU, IL, LI, W))
    b, h = np.asarray(b, np.float64).reshape(-1), np.asarray(h, np.float64).reshape(-1)
    I = IU.shape[0]
    out = np.empty((len(users), I))
    every = np.arange(I)
    for k, u in enumerate(users):
        out[k] = scores(UI, IU, IL, LI, W, b, h, np.full(I, u), every, np.tile(np.asarray(last[u], np.int64), (I, 1)))
    return out


def edge_patterns(users, recents, items, third, pairwise):
    """the duplicate patterns a golden batch holds: a user twice; an item that is the target of one instance and a
    recent of another; an item twice among one instance's recents; pairwise: a negative that is another instance's
    positive"""
    users, items = np.asarray(users).tolist(), np.asarray(items).tolist()
    rec = np.asarray(recents).reshape(len(users), -1)
    out = {"user twice": len(set(users)) < len(users),
           "recent and target": bool(set(rec.reshape(-1).tolist()) & set(items)),
           "item twice in a window": any(len(set(r)) < len(r) for r in rec.tolist())}
    if pairwise:
        negs = np.asarray(third).tolist()
        out["negative is a positive"] = any(j in set(items[:k] + items[k + 1:]) for k, j in enumerate(negs))
    return out
