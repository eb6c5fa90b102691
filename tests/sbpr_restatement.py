"""A float64 numpy restatement of SBPR (model/social_recommender/SBPR.py, util/learner.py, TF-1.12's sparse optimiser
kernels) for the SBPR tests: the social item sets with their counts, the rules an epoch's instances obey, the
gradients of one batch by hand and one training step for every loss and learner, and predict().
Checked against the reference class's own sets, suk and f64 trace in test_sbpr_cpu.py; the GPU tests use it for the
shapes and graphs the trace does not hold."""
import numpy as np

import fism_restatement as F

TABLES = ("P", "Q", "b")
REG = 0.01
# case -> (loss, learner); `bpr_adam_dup`: one item as i, k and j of different slots, a user several times
CASES = {"bpr_adam": ("bpr", "adam"), "hinge_gd": ("hinge", "gd"), "square_adagrad": ("square", "adagrad"),
         "bpr_rmsprop": ("bpr", "rmsprop"), "bpr_momentum": ("bpr", "momentum"), "bpr_adam_dup": ("bpr", "adam")}
STEPS = {"bpr_adam": 3, "bpr_adam_dup": 1}                 # every other case: 2
PREDICT_CASE = "bpr_adam"


# ------------------------------------------------------------------ inputs
def trust_graph(train, seed=2019, every_empty=11, only_train_users=True):
    """a seeded directed trust graph over the users of `train` (CSR) as (user, friend) LINES: out-degree
    round(lognormal(1.2, 0.8)), every `every_empty`-th user trusts nobody, every 7th of the others trusts themself,
    every 5th line is written twice.  only_train_users: trusted users are drawn among the users with train items"""
    rs = np.random.RandomState(seed)
    U = train.shape[0]
    deg_tr = np.diff(train.indptr)
    pool = np.flatnonzero(deg_tr > 0) if only_train_users else np.arange(U)
    lines = []
    for u in range(U):
        deg = int(round(rs.lognormal(1.2, 0.8)))
        friends = rs.choice(pool, min(deg, len(pool)), replace=False).tolist()
        if u % every_empty == 0:
            continue
        if u % 7 == 3 and (deg_tr[u] > 0 or not only_train_users):
            friends.append(u)
        for f in friends:
            lines.append((u, int(f)))
            if len(lines) % 5 == 0:
                lines.append((u, int(f)))
    return lines


def trust_csr(lines, n_users):
    """(int64 indptr, int32 indices) of the deduplicated trust matrix, indices ascending per row"""
    pairs = sorted(set((int(u), int(f)) for u, f in lines))
    indptr = np.zeros(n_users + 1, np.int64)
    for u, _ in pairs:
        indptr[u + 1] += 1
    return np.cumsum(indptr), np.asarray([f for _, f in pairs], np.int32)


# ------------------------------------------------------------------ the sets and the instance rules
def social_sets(tr_indptr, tr_indices, s_indptr, s_indices):
    """{u: (items ascending, counts)} for the users with train items and a non-empty set (SBPR.py:40-49): count = the
    number of trusted users who hold the item = suk - 1 (SBPR.py:143-145).  A trusted user without train items adds
    nothing"""
    out = {}
    for u in range(len(tr_indptr) - 1):
        own = set(tr_indices[tr_indptr[u]:tr_indptr[u + 1]].tolist())
        if not own:
            continue
        cnt = {}
        for f in s_indices[s_indptr[u]:s_indptr[u + 1]].tolist():
            for k in tr_indices[tr_indptr[f]:tr_indptr[f + 1]].tolist():
                if k not in own:
                    cnt[k] = cnt.get(k, 0) + 1
        if cnt:
            items = sorted(cnt)
            out[u] = (np.asarray(items, np.int32), np.asarray([cnt[k] for k in items], np.int32))
    return out


def sets_as_csr(sets, n_users):
    indptr = np.zeros(n_users + 1, np.int64)
    for u, (items, _) in sets.items():
        indptr[u + 1] = len(items)
    order = sorted(sets)
    cat = lambda c: np.concatenate([sets[u][c] for u in order]).astype(np.int32) if order else np.zeros(0, np.int32)
    return np.cumsum(indptr), cat(0), cat(1)


def check_no_free_item(tr_indptr, sets, n_items):
    """the refusal of an eligible user whose train items and social items are all the items"""
    for u, (items, _) in sorted(sets.items()):
        if int(tr_indptr[u + 1] - tr_indptr[u]) + len(items) >= n_items:
            raise ValueError("SBPR: user %d has no item outside its train items and its social items: no negative "
                             "can be drawn" % u)


def eligible_positives(tr_indptr, tr_indices, sets):
    """[(u, i)] in the order of SBPR.py:126-132: train_dict order, every train item of an eligible user"""
    return [(u, int(i)) for u in sorted(sets) for i in tr_indices[tr_indptr[u]:tr_indptr[u + 1]]]


# ------------------------------------------------------------------ the step
class State(F.State):
    """the optimiser state of fism_restatement on SBPR's three tables; b as a vector"""

    def __init__(self, P, Q, b, learner="adam", lr=0.01, momentum=0.9):
        f = lambda x: np.array(x, dtype=np.float64)
        self.var = {"P": f(P), "Q": f(Q), "b": f(b).reshape(-1)}
        self.learner, self.lr, self.momentum = learner, lr, momentum
        init = {"adam": 0.0, "gd": 0.0, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        self.s0 = {k: np.full_like(v, init) for k, v in self.var.items()}
        self.s1 = {k: np.zeros_like(v) for k, v in self.var.items()}
        self.b1p, self.b2p = 0.9, 0.999

    def tables(self):
        return [self.var[k] for k in TABLES]


def golden_tables(g, case, tag, step):
    """(P, Q, b) of the trace after `step` (0-based; -1: the initial ones), full size, in the trace's width"""
    dt = np.float32 if tag == "f32" else np.float64
    out = []
    for name in TABLES:
        t = g[name + "_0"].astype(np.float64)
        if step >= 0:
            rows = g["%s_rows_%s" % (case, name)]
            t[rows] = t[rows] + g["%s_%s_%s" % (case, tag, name)][step]
        out.append(t.astype(dt))
    return out


def loss_and_slope(loss, y):
    """util/learner.py:19-29 per element and its derivative"""
    if loss == "bpr":
        return np.logaddexp(0.0, -y), -1.0 / (1.0 + np.exp(y))
    if loss == "hinge":
        return np.maximum(y + 1, 0), (y + 1 > 0).astype(np.float64)
    return (1 - y) ** 2, -2.0 * (1 - y)


def gradients(P, Q, b, users, items, social, negatives, suk, loss, reg):
    """(loss, {table: gradient}) of one batch: SBPR.py:68-88 and its derivative by hand.  P_u enters the regulariser
    once per slot; a row that occurs twice in the batch is counted twice"""
    u, i, k, j = (np.asarray(x, np.int64) for x in (users, items, social, negatives))
    s = np.asarray(suk, np.float64)
    x = lambda a: (P[u] * Q[a]).sum(axis=1) + b[a]
    y1, y2 = (x(i) - x(k)) / s, x(k) - x(j)
    (l1, d1), (l2, d2) = loss_and_slope(loss, y1), loss_and_slope(loss, y2)
    sq = (P[u] ** 2).sum() + sum((Q[a] ** 2).sum() + (b[a] ** 2).sum() for a in (i, k, j))
    total = l1.sum() + l2.sum() + reg * 0.5 * sq
    g1, g2 = d1 / s, d2
    G = {"P": np.zeros_like(P), "Q": np.zeros_like(Q), "b": np.zeros_like(b)}
    np.add.at(G["P"], u, g1[:, None] * Q[i] + (g2 - g1)[:, None] * Q[k] - g2[:, None] * Q[j] + reg * P[u])
    for a, c in ((i, g1), (k, g2 - g1), (j, -g2)):
        np.add.at(G["Q"], a, c[:, None] * P[u] + reg * Q[a])
        np.add.at(G["b"], a, c + reg * b[a])
    return total, G


def touched(users, items, social, negatives):
    ijk = np.unique(np.concatenate([np.asarray(x, np.int64) for x in (items, social, negatives)]))
    return {"P": np.unique(np.asarray(users, np.int64)), "Q": ijk, "b": ijk}


def step(st, users, items, social, negatives, suk, loss, reg):
    """one sess.run((loss, optimizer)): returns the pre-update loss"""
    total, G = gradients(*st.tables(), users, items, social, negatives, suk, loss, reg)
    for name, rows in touched(users, items, social, negatives).items():
        st.apply(name, G[name], rows)
    st.b1p, st.b2p = st.b1p * 0.9, st.b2p * 0.999
    return float(total)


def predict(P, Q, users):
    """SBPR.py:155-158: P_u . Q_j, WITHOUT the bias"""
    return np.asarray(P, np.float64)[np.asarray(users, np.int64)] @ np.asarray(Q, np.float64).T
