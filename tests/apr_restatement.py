"""A numpy restatement of APR (model/general_recommender/APR.py:73-118, util/learner.py, TF-1.12's optimiser kernels)
for the APR tests, in the width of the tables it is given: the plain gradient of a batch, Delta, the gradient of
opt_loss with Delta constant, and one training step in every learner form.  Checked against the reference class's own
f64 trace and against torch autograd in test_apr_cpu.py; the GPU tests use it for the shapes the trace does not hold.

    x_t = <P[u], Q[i]> - <P[u], Q[j]>      loss = sum softplus(-x_t)      s_t = -sigmoid(-x_t)
    Delta[row] = eps * Gamma[row] * rsqrt(max(|Gamma[row]|^2, 1e-12)),  Gamma = d loss / d row
    opt_loss = loss + reg * (sum(P^2) / 2 + sum(Q^2) / 2) + reg_adv * sum softplus(-x~_t)
"""
import numpy as np

# case -> (adv: "grad" / "random" / None for adver = 0 / "shipped" for the class's own optimizer, learner, d, reg,
#          reg_adv, eps)
CASES = {"grad_adam": ("grad", "adam", 16, 0.0, 1.0, 0.5),
         "grad_reg_gd": ("grad", "gd", 7, 0.05, 0.5, 0.1),
         "grad_adagrad": ("grad", "adagrad", 33, 0.0, 1.0, 0.5),
         "random_adam": ("random", "adam", 9, 0.0, 1.0, 0.5),
         "plain_reg_adam": (None, "adam", 16, 0.05, 1.0, 0.5),
         "shipped_adam": ("shipped", "adam", 16, 0.05, 1.0, 0.5)}
STEPS = 3
BATCH = 48
LR = 0.01
LEARNERS = ("adam", "gd", "adagrad", "rmsprop", "momentum")


def adversarial_epochs(epochs, adver, adv_epoch, reference_train_loop):
    """the 1-based epochs whose steps perturb"""
    if reference_train_loop or not adver:
        return []
    return [e for e in range(1, epochs + 1) if e > adv_epoch]


def valid(P, Q, users, pos, neg):
    u, i, j = (np.asarray(x, np.int64) for x in (users, pos, neg))
    ok = (u >= 0) & (u < len(P)) & (i >= 0) & (i < len(Q)) & (j >= 0) & (j < len(Q))
    return u[ok], i[ok], j[ok]


def softplus(x):
    return np.logaddexp(np.zeros_like(x), x)


def _pass(P, Q, pu, qi, qj, u, i, j, scale):
    """loss and d(scale * loss) of the pairs' rows pu / qi / qj scattered to tables of the shapes of P and Q"""
    x = (pu * qi).sum(axis=1) - (pu * qj).sum(axis=1)
    s = (-scale / (1.0 + np.exp(x)))[:, None]
    GP, GQ = np.zeros_like(P), np.zeros_like(Q)
    np.add.at(GP, u, s * (qi - qj))
    np.add.at(GQ, i, s * pu)
    np.add.at(GQ, j, -s * pu)
    return softplus(-x).sum(), GP, GQ


def normalise(G, eps):
    """tf.nn.l2_normalize(G, 1) * eps"""
    n2 = (G * G).sum(axis=1, keepdims=True)
    return G * (1.0 / np.sqrt(np.maximum(n2, 1e-12))) * eps


def batch_rows(P, Q, users, pos, neg):
    u, i, j = valid(P, Q, users, pos, neg)
    return np.unique(u), np.unique(np.concatenate([i, j]))


def gradients(P, Q, users, pos, neg, reg=0.0, reg_adv=1.0, eps=0.5, adversarial=True, with_reg=True, delta=None):
    """(loss, opt_loss, G_P, G_Q, Delta_P, Delta_Q): the dense gradient of opt_loss with Delta constant.  delta: (Delta_P,
    Delta_Q) whole tables in place of the gradient's own (the `random` mode's draw); not adversarial: the adver = 0
    graph.  with_reg False: loss alone (the loop as shipped)"""
    u, i, j = valid(P, Q, users, pos, neg)
    loss, GP, GQ = _pass(P, Q, P[u], Q[i], Q[j], u, i, j, 1.0)
    opt, dP, dQ = loss, np.zeros_like(P), np.zeros_like(Q)
    if adversarial:
        dP, dQ = (normalise(GP, eps), normalise(GQ, eps)) if delta is None else delta
        loss_adv, AP, AQ = _pass(P, Q, P[u] + dP[u], Q[i] + dQ[i], Q[j] + dQ[j], u, i, j, reg_adv)
        opt, GP, GQ = opt + reg_adv * loss_adv, GP + AP, GQ + AQ
    if with_reg:
        opt = opt + reg * ((P * P).sum() / 2 + (Q * Q).sum() / 2)
        GP, GQ = GP + reg * P, GQ + reg * Q
    return loss, opt, GP, GQ, dP, dQ


class State:
    """the two tables and their optimiser slots as TF creates them"""

    def __init__(self, P, Q, learner="adam", lr=LR, momentum=0.9, dtype=np.float64):
        self.P, self.Q = np.array(P, dtype=dtype), np.array(Q, dtype=dtype)
        self.learner, self.lr, self.momentum, self.dtype = learner, lr, momentum, dtype
        init = {"adam": 0.0, "gd": 0.0, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        self.s0 = [np.full_like(self.P, init), np.full_like(self.Q, init)]
        self.s1 = [np.zeros_like(self.P), np.zeros_like(self.Q)]
        self.b1p, self.b2p = dtype(0.9), dtype(0.999)

    def apply(self, k, var, g, rows):
        """rows None: the dense Apply* kernel; else the sparse one on `rows` (Adam's sparse form sweeps every row)"""
        s0, s1, lr, f = self.s0[k], self.s1[k], self.dtype(self.lr), self.dtype
        r = slice(None) if rows is None else rows
        if self.learner == "adam":
            alpha = lr * np.sqrt(f(1) - self.b2p) / (f(1) - self.b1p)
            if rows is None:
                s0 += (g - s0) * (f(1) - f(0.9))
                s1 += (g * g - s1) * (f(1) - f(0.999))
                var -= (s0 * alpha) / (np.sqrt(s1) + f(1e-8))
            else:
                s0[:] = s0 * f(0.9) + g * (f(1) - f(0.9))
                s1[:] = s1 * f(0.999) + (g * g) * (f(1) - f(0.999))
                var -= alpha * s0 / (np.sqrt(s1) + f(1e-8))
        elif self.learner == "gd":
            var[r] -= lr * g[r]
        elif self.learner == "adagrad":
            s0[r] += g[r] * g[r]
            var[r] -= (lr * g[r]) * (f(1) / np.sqrt(s0[r]))
        elif self.learner == "rmsprop":
            if rows is None:
                s0 += (g * g - s0) * (f(1) - f(0.9))
                s1[:] = s1 * f(0.0) + (g * lr) / np.sqrt(f(1e-10) + s0)
            else:
                s0[r] = s0[r] * f(0.9) + (g[r] * g[r]) * (f(1) - f(0.9))
                s1[r] = s1[r] * f(0.0) + (f(1) / np.sqrt(s0[r] + f(1e-10))) * lr * g[r]
            var[r] -= s1[r]
        else:
            s0[r] = s0[r] * f(self.momentum) + g[r]
            var[r] -= s0[r] * lr

    def finish(self):
        self.b1p, self.b2p = self.b1p * self.dtype(0.9), self.b2p * self.dtype(0.999)


def step(st, users, pos, neg, reg=0.0, reg_adv=1.0, eps=0.5, adversarial=True, with_reg=True, delta=None, dense=None):
    """one optimiser step: (loss, opt_loss, Delta_P, Delta_Q) at the incoming tables.  dense None: the engine's rule —
    the dense application when the regulariser reads the tables (with_reg and reg != 0), else the sparse one on the
    batch's rows"""
    loss, opt, GP, GQ, dP, dQ = gradients(st.P, st.Q, users, pos, neg, reg, reg_adv, eps, adversarial, with_reg, delta)
    if dense is None:
        dense = bool(with_reg) and reg != 0.0
    rows = (None, None) if dense else batch_rows(st.P, st.Q, users, pos, neg)
    st.apply(0, st.P, GP, rows[0])
    st.apply(1, st.Q, GQ, rows[1])
    st.finish()
    return loss, opt, dP, dQ


def edge_patterns(users, pos, neg):
    """what every golden batch holds: a user three times, an item that is positive in one triplet and negative in
    another, a (user, positive) pair twice"""
    u, i, j = (np.asarray(x).tolist() for x in (users, pos, neg))
    pairs = list(zip(u, i))
    return {"user_three_times": max(u.count(a) for a in set(u)) >= 3,
            "item_in_both_roles": bool(set(i) & set(j)),
            "pair_twice": max(pairs.count(p) for p in set(pairs)) >= 2}


def golden_tables(g, case, tag, step_):
    """(P, Q) of the trace after `step_` (0-based; -1: the initial ones), whole, in float64"""
    out = []
    for name in ("P", "Q"):
        t = g["%s_%s_0" % (case, name)].astype(np.float64)
        if step_ >= 0:
            rows = g["%s_rows_%s" % (case, name)]
            t[rows] = t[rows] + g["%s_%s_%s" % (case, tag, name)][step_]
        out.append(t)
    return out


def golden_delta(g, case, tag, step_, shapes):
    """(Delta_P, Delta_Q) of the trace's step as whole tables in float64: zero outside the batch's rows"""
    out = []
    for name, shape in zip(("P", "Q"), shapes):
        t = np.zeros(shape, np.float64)
        t[g["%s_drows_%s_%d" % (case, name, step_)]] = g["%s_%s_delta_%s_%d" % (case, tag, name, step_)]
        out.append(t)
    return out
