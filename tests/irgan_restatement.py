"""IRGAN restated in numpy (float64 by default, float32 on request) from the formulas of the reference's graph
(model/general_recommender/IRGAN.py), and the device's weights and draw rules in Python integers.

    D step   sum_b ce(y_b, <P_u, Q_i> + b_i) + B d_reg / 2 (sum_b |P_u|^2 + sum_b |Q_i|^2 + sum_b b_i^2)
             (`minimize` of the vector pre_loss differentiates its sum: the scalar regulariser counts B times)
    G step   p = softmax(Q P_u + b); pn = 0.8 p + 0.2 / deg on the positives; r_s = 2 (sigmoid(D's logit) - 1/2) p / pn;
             -mean_s(r_s log p[i_s]) + g_reg / 2 (|P_u|^2 + sum_s |Q_{i_s}|^2 + sum_s b_{i_s}^2), r held constant
"""
import numpy as np

MASK64 = (1 << 64) - 1
LR, BATCH, FACTORS = 0.05, 8, 5
# name: (g_reg, d_reg, d_tau, d_epoch, g_epoch)
CASES = {"defaults": (0.0, 0.1 / 16, 0.2, 1, 1), "greg": (0.03, 0.02, 1.0, 1, 1), "steps": (0.01, 0.1 / 16, 0.2, 2, 2)}
NAMES = ("g_P", "g_Q", "g_b", "d_P", "d_Q", "d_b")


def init_tables(n_users, n_items, d, seed):
    """the six tables: G as a pretrained pickle would give it (a bias that is not zero), D uniform(-0.05, 0.05) with a
    zero bias (IRGAN.py:79-85)"""
    rs = np.random.RandomState(seed)
    out = {"g_P": rs.uniform(-0.5, 0.5, (n_users, d)), "g_Q": rs.uniform(-0.5, 0.5, (n_items, d)),
           "g_b": rs.uniform(-0.3, 0.3, n_items), "d_P": rs.uniform(-0.05, 0.05, (n_users, d)),
           "d_Q": rs.uniform(-0.05, 0.05, (n_items, d)), "d_b": np.zeros(n_items)}
    return {k: v.astype(np.float32) for k, v in out.items()}


def train_users(indptr, indices):
    """IRGAN.py:142-147: the rows for which any(row.indices) — not the empty ones, not [0] alone"""
    return [u for u in range(len(indptr) - 1) if any(indices[indptr[u]:indptr[u + 1]])]


# ------------------------------------------------------------------ the generator of csrc/nr_core.h in Python integers
def splitmix64(x):
    x = (x + 0x9e3779b97f4a7c15) & MASK64
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & MASK64
    return x ^ (x >> 31)


def draw_words(seed, pas, phase, user, s):
    """the three hash words of draw s: nr::XorShift64s seeded with (seed, ((pass << 2 | phase) << 32) | user, s)"""
    stream = ((((pas << 2) | (phase & 3)) << 32) | (user & 0xffffffff)) & MASK64
    z = splitmix64(seed ^ splitmix64((stream * 0xd1342543de82ef95 + 0x632be59bd9b4e019) & MASK64))
    z = splitmix64(z ^ ((s * 0x9e3779b97f4a7c15) & MASK64))
    st = z if z else 0x2545f4914f6cdd1d
    out = []
    for _ in range(3):
        st ^= st >> 12
        st = (st ^ (st << 25)) & MASK64
        st ^= st >> 27
        out.append((st * 0x2545f4914f6cdd1d) & MASK64)
    return out


def weights(z, tau, dtype=np.float64):
    """w_i = floor(exp((z_i - max z) / tau) 2^31), in `dtype` arithmetic"""
    z = np.asarray(z, dtype)
    e = np.exp((z - z.max()) / dtype(tau))
    return np.floor(e.astype(np.float64) * 2.0 ** 31).astype(np.uint64)


def _find(x, cum):
    """the smallest i whose inclusive prefix sum exceeds x"""
    lo, hi = 0, len(cum) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if cum[mid] > x:
            hi = mid
        else:
            lo = mid + 1
    return lo


def _cum(w):
    out, acc = [], 0
    for v in w:
        acc += int(v)
        out.append(acc)
    return out


def plain_draws(w, n, seed, pas, user):
    """phase 0: n draws from the weights"""
    cum = _cum(w)
    return np.asarray([_find((draw_words(seed, pas, 0, user, s)[0] * cum[-1]) >> 64, cum) for s in range(n)], np.int32)


def mixture_draws(w, pos, seed, pas, user):
    """phase 1: 2 deg draws from 0.8 w / W + 0.2 / deg on the positives"""
    cum, deg, out = _cum(w), len(pos), []
    for s in range(2 * deg):
        h = draw_words(seed, pas, 1, user, s)
        if (h[0] * 5) >> 64 == 0:
            out.append(int(pos[(h[1] * deg) >> 64]))
        else:
            out.append(_find((h[2] * cum[-1]) >> 64, cum))
    return np.asarray(out, np.int32)


def d_data(P, Q, b, indptr, indices, tau, seed, pas, users=None, dtype=np.float64):
    """the interleaved (u, pos_k, 1), (u, draw_k, 0) of every train user, ascending"""
    us, its, ys = [], [], []
    for u in (train_users(indptr, indices) if users is None else users):
        pos = indices[indptr[u]:indptr[u + 1]]
        w = weights(np.asarray(Q, dtype) @ np.asarray(P, dtype)[u] + np.asarray(b, dtype), tau, dtype)
        for i, j in zip(pos, plain_draws(w, len(pos), seed, pas, u)):
            us += [u, u]
            its += [int(i), int(j)]
            ys += [1.0, 0.0]
    return np.asarray(us, np.int32), np.asarray(its, np.int32), np.asarray(ys, np.float32)


# ------------------------------------------------------------------ the two steps
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


class IRGAN:
    def __init__(self, tables, indptr, indices, lr, g_reg, d_reg, dtype=np.float64):
        self.dt = dtype
        self.T = {k: np.asarray(tables[k], np.float32).astype(dtype).copy() for k in NAMES}
        self.indptr, self.indices = np.asarray(indptr), np.asarray(indices)
        self.lr, self.g_reg, self.d_reg = dtype(lr), dtype(g_reg), dtype(d_reg)

    def pos(self, u):
        return self.indices[self.indptr[u]:self.indptr[u + 1]]

    def d_gradients(self, users, items, labels):
        """((ce sum, B d_reg / 2 (|P|^2 + |Q|^2), B d_reg / 2 b^2), {table: dense gradient})"""
        dt, T = self.dt, self.T
        users, items, y = np.asarray(users, np.int64), np.asarray(items, np.int64), np.asarray(labels, dt)
        P, Q, b = T["d_P"], T["d_Q"], T["d_b"]
        breg = dt(len(users)) * self.d_reg
        x = (P[users] * Q[items]).sum(1) + b[items]
        e = _sigmoid(x) - y
        ce = np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))
        terms = (ce.sum(), breg * ((P[users] ** 2).sum() + (Q[items] ** 2).sum()) / 2, breg * (b[items] ** 2).sum() / 2)
        G = {k: np.zeros_like(T[k]) for k in ("d_P", "d_Q", "d_b")}
        np.add.at(G["d_P"], users, e[:, None] * Q[items] + breg * P[users])
        np.add.at(G["d_Q"], items, e[:, None] * P[users] + breg * Q[items])
        np.add.at(G["d_b"], items, e + breg * b[items])
        return terms, G

    def d_step(self, users, items, labels):
        if len(users) == 0:
            return (0.0, 0.0, 0.0)
        terms, G = self.d_gradients(users, items, labels)
        for k, g in G.items():
            self.T[k] = (self.T[k] - self.lr * g).astype(self.dt)
        return terms

    def rewards(self, user, samples):
        """(p, r): the generator's softmax for `user`, and r_s = 2 (sigmoid(D's logit) - 1/2) p / pn"""
        dt, T = self.dt, self.T
        samples, pos = np.asarray(samples, np.int64), self.pos(user)
        z = T["g_Q"] @ T["g_P"][user] + T["g_b"]
        e = np.exp(z - z.max())
        p = e / e.sum()
        pn = dt(0.8) * p
        pn[pos] += dt(0.2) / dt(len(pos))
        x = (T["d_P"][user] * T["d_Q"][samples]).sum(1) + T["d_b"][samples]
        return p, dt(2) * (_sigmoid(x) - dt(0.5)) * p[samples] / pn[samples]

    def g_gradients(self, user, samples):
        """{table: dense gradient} of the G loss at the recorded samples, r held constant"""
        T, I = self.T, len(self.T["g_b"])
        samples = np.asarray(samples, np.int64)
        S = self.dt(len(samples))
        p, r = self.rewards(user, samples)
        c = np.bincount(samples, minlength=I).astype(self.dt)
        dz = ((r.sum() * p - np.bincount(samples, weights=r, minlength=I).astype(self.dt)) / S).astype(self.dt)
        G = {"g_P": np.zeros_like(T["g_P"]), "g_Q": np.outer(dz, T["g_P"][user]) + self.g_reg * c[:, None] * T["g_Q"],
             "g_b": dz + self.g_reg * c * T["g_b"]}
        G["g_P"][user] = T["g_Q"].T @ dz + self.g_reg * T["g_P"][user]
        return G

    def g_step(self, user, samples):
        for k, g in self.g_gradients(user, samples).items():
            self.T[k] = (self.T[k] - self.lr * g).astype(self.dt)

    def ratings(self):
        return self.T["g_P"] @ self.T["g_Q"].T + self.T["g_b"]
