"""A float64 numpy restatement of FISM (FISM.py:55-92, util/learner.py, TF-1.12's optimiser kernels) for the FISM tests:
the instance rule, one training step for every learner (dense application for c1, row application for Q and bias) and
predict().  Checked against the reference class's own f64 trace in test_fism_cpu.py; the GPU tests use it for the
shapes the trace does not hold."""
import numpy as np
import scipy.sparse as sp


def golden_matrix(g):
    U, I = (int(x) for x in g["shape"])
    return sp.csr_matrix((np.ones(len(g["indices"]), np.float32), g["indices"], g["indptr"]), shape=(U, I))


def golden_tables(g, case, tag, step):
    """(c1, Q, bias) of the trace after `step` (0-based), full size, in the trace's width"""
    dt = np.float32 if tag == "f32" else np.float64
    out = []
    for name, init in (("c1", g["c1_0"]), ("Q", g["Q0"]), ("bias", g["bias_0"])):
        t = init.astype(np.float64)
        rows = g["%s_rows_%s" % (case, name)]
        t[rows] = t[rows] + g["%s_%s_%s" % (case, tag, name)][step]
        out.append(t.astype(dt))
    return out


def instances(R, users, items, third, pairwise):
    """[(user, item, excluded or -1, n, regularise p?)] by util/data_generator.py:29-54: pointwise one per slot;
    pairwise the positive sides, then the negative sides, users with one train item dropped"""
    deg = np.diff(R.indptr)
    if not pairwise:
        return [(int(u), int(i), int(i) if y > 0.5 else -1, int(deg[u]) if y > 0.5 else int(deg[u]) + 1, True)
                for u, i, y in zip(users, items, third)]
    keep = [k for k, u in enumerate(users) if deg[u] > 1]
    return [(int(users[k]), int(items[k]), int(items[k]), int(deg[users[k]]), True) for k in keep] + \
           [(int(users[k]), int(third[k]), -1, int(deg[users[k]]) + 1, False) for k in keep]


def history(R, u, excl):
    row = R.indices[R.indptr[u]:R.indptr[u + 1]]
    return row[row != excl]


class State:
    def __init__(self, c1, Q, bias=None, learner="adam", lr=0.01, momentum=0.9):
        f = lambda x: np.array(x, dtype=np.float64)
        self.var = {"c1": f(c1), "Q": f(Q), "bias": f(np.zeros(len(Q)) if bias is None else bias)}
        self.learner, self.lr, self.momentum = learner, lr, momentum
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


def step(st, R, users, items, third, pairwise, loss, alpha, regs, c1_rows=False):
    """one sess.run((loss, optimizer)): returns the pre-update loss.  c1_rows: c1 gets the sparse application on the
    rows the batch's histories hold instead of the dense one"""
    c1, Q, bias = st.var["c1"], st.var["Q"], st.var["bias"]
    inst = instances(R, users, items, third, pairwise)
    N = len(inst)
    p = np.stack([c1[history(R, u, e)].sum(axis=0) for u, _, e, _, _ in inst]) if N else np.zeros((0, c1.shape[1]))
    it = np.asarray([i for _, i, _, _, _ in inst], np.int64)
    coeff = np.asarray([float(n) ** -alpha for _, _, _, n, _ in inst])
    regp = np.asarray([1.0 if r else 0.0 for _, _, _, _, r in inst])
    out = coeff * (p * Q[it]).sum(axis=1) + bias[it]
    if not pairwise:
        y = np.asarray(third, np.float64)
        if loss == "square":
            total, dout = ((y - out) ** 2).sum(), -2.0 * (y - out)
        else:
            total = (np.maximum(out, 0) - out * y + np.log1p(np.exp(-np.abs(out)))).mean()
            dout = (1.0 / (1.0 + np.exp(-out)) - y) / N
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
    total += regs[0] * 0.5 * (regp[:, None] * p * p).sum() + regs[1] * 0.5 * (Q[it] ** 2).sum()
    g = (dout * coeff)[:, None] * Q[it] + regs[0] * regp[:, None] * p
    G_c1, G_Q, G_b = np.zeros_like(c1), np.zeros_like(Q), np.zeros_like(bias)
    for b, (u, _, e, _, _) in enumerate(inst):
        G_c1[history(R, u, e)] += g[b]
    np.add.at(G_Q, it, (dout * coeff)[:, None] * p + regs[1] * Q[it])
    np.add.at(G_b, it, dout)
    rows = np.unique(it)
    hist = [history(R, u, e) for u, _, e, _, _ in inst]
    st.apply("c1", G_c1, np.unique(np.concatenate(hist)).astype(np.int64) if (c1_rows and hist) else None)
    st.apply("Q", G_Q, rows)
    st.apply("bias", G_b, rows)
    st.b1p, st.b2p = st.b1p * 0.9, st.b2p * 0.999
    return total


def predict(R, c1, Q, bias, users, alpha):
    """FISM.py:168-179: the whole train row, n = |R_u|, every item; a user without train items scores the bias"""
    c1, Q, bias = (np.asarray(x, np.float64) for x in (c1, Q, bias))
    out = np.empty((len(users), Q.shape[0]))
    for k, u in enumerate(users):
        row = R.indices[R.indptr[u]:R.indptr[u + 1]]
        out[k] = (float(len(row)) ** -alpha * (Q @ c1[row].sum(axis=0)) if len(row) else 0.0) + bias
    return out
