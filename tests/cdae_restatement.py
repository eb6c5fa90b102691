"""CDAE restated in numpy: the batch of CDAE.py:108-140 given the draws, the loss of CDAE.py:62-96 with its
gradients, TF-1.12 Adam, predict(), and — bit for bit — the device's counter-based draw and mask generators
(csrc/nr_core.h XorShift64s / draw_negative, csrc/cdae.hip mask_draw).  float64 unless a dtype is asked for."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15
SEGMENT_DRAWS = 16384
TABLES = ("user_embeddings", "en_embeddings", "en_offset", "de_embeddings", "de_bias")

# the cases of tests/golden/tfgraph_cdae.npz: (hidden_act, loss_func, reg, dropout, hidden_dim)
CASES = {"default": ("sigmoid", "sigmoid_cross_entropy", 0.01, 0.5, 8),
         "ident_sq": ("identity", "square", 0.0, 0.0, 7),
         "sig_sq": ("sigmoid", "square", 0.02, 0.5, 5),
         "ident_ce": ("identity", "sigmoid_cross_entropy", 0.0, 0.5, 9)}
EPOCH_CASE, LR, NUM_NEG = "default", 0.001, 3


def keep_of(uniforms, dropout):
    """dropout_sparse's flag in float32: floor(u + keep) == 1, keep = 1 - dropout"""
    keep = np.float32(1.0) - np.float32(dropout)
    return (np.floor(np.asarray(uniforms, np.float32) + keep) == 1).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- the generators
def splitmix64(x):
    x = (x + GOLDEN) & M64
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & M64
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


class XorShift64s:
    def __init__(self, key, stream, counter):
        z = splitmix64(key ^ splitmix64((stream * 0xd1342543de82ef95 + 0x632be59bd9b4e019) & M64))
        z = splitmix64(z ^ ((counter * GOLDEN) & M64))
        self.s = z if z else 0x2545f4914f6cdd1d

    def next(self):
        s = self.s
        s ^= s >> 12
        s = (s ^ (s << 25)) & M64
        s ^= s >> 27
        self.s = s
        return (s * 0x2545f4914f6cdd1d) & M64


def draw_negative(g, high, excl, have=None):
    """nr::draw_negative: excl ascending (have: the same as a set); -1 when nothing is allowed"""
    n = len(excl)
    if n >= high:
        return -1
    have = set(int(x) for x in excl) if have is None else have
    for _ in range(64):
        a = g.next() % high
        if a not in have:
            return int(a)
    r = g.next() % (high - n)
    lo = int(np.searchsorted(np.asarray(excl, np.int64) - np.arange(n), r, side="right"))
    return int(r + lo)


def draws(seed, user, row, n_items, count):
    """the first `count` draws of `user` under `seed`: whatever batch the user is in"""
    have = set(int(x) for x in row)
    return np.asarray([draw_negative(XorShift64s(seed & M64, int(user), q), n_items, row, have) for q in range(count)],
                      dtype=np.int64)


def negatives(seed, users, indptr, indices, n_items, num_neg):
    """per slot: np.unique of the user's |R_u| num_neg draws"""
    out = []
    for u in users:
        row = indices[indptr[u]:indptr[u + 1]]
        d = draws(seed, u, row, n_items, len(row) * num_neg)
        out.append(np.unique(d[d >= 0]).astype(np.int32))
    return out


def mask(seed, step, n, keep):
    """uint8 [n]: the drawn corruption mask of entries 0..n-1 (float32 compare, as on the device)"""
    key = splitmix64((seed & M64) ^ ((step * GOLDEN + 0x6e6f6465) & M64))
    u = np.asarray([splitmix64(key ^ e) >> 40 for e in range(n)], dtype=np.float32) * np.float32(1.0 / 16777216.0)
    return (u < np.float32(keep)).astype(np.uint8)


def step_seed(seed, t):
    """CDAEEngine.step_seed: the draws of the step after t applied ones"""
    return (seed + GOLDEN * (t + 1)) & M64


# ---------------------------------------------------------------------------------------------- test data
def init_tables(U, I, d, seed, scale=0.1):
    """the five variables, float32; offset and bias non-zero so that their terms show"""
    rs = np.random.RandomState(seed)
    shapes = {"user_embeddings": (U, d), "en_embeddings": (I, d), "en_offset": (d,), "de_embeddings": (I, d),
              "de_bias": (I,)}
    return {k: (scale * rs.standard_normal(s)).astype(np.float32) for k, s in shapes.items()}


def csr_of(rows, n_items):
    """(indptr int64, indices int32, scipy CSR) of the given item lists, one per user, sorted"""
    import scipy.sparse as sp
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate([np.sort(np.asarray(r, np.int32)) for r in rows]).astype(np.int32) if len(rows) \
        else np.zeros(0, np.int32)
    M = sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(len(rows), n_items))
    return indptr, indices, M


def random_rows(sizes, n_items, seed):
    rs = np.random.RandomState(seed)
    return [np.sort(rs.choice(n_items, n, replace=False)) for n in sizes]


# ---------------------------------------------------------------------------------------------- the batch
def build_batch(indptr, indices, users, negs):
    """CDAE.py:113-132: per slot the positives ascending (label 1) then the negatives ascending (label 0); the input
    entries row-major with ascending columns (tocoo of a CSR); in_pos[e]: where entry e's item sits in the input"""
    ptr, items, labels, slot, in_items, in_pos = [0], [], [], [], [], []
    for s, u in enumerate(users):
        row = np.asarray(indices[indptr[u]:indptr[u + 1]], np.int64)
        dec = np.concatenate([row, np.asarray(negs[s], np.int64)])
        merged = np.sort(dec)
        items.append(dec)
        labels.append(np.concatenate([np.ones(len(row)), np.zeros(len(negs[s]))]))
        slot.append(np.full(len(dec), s, np.int64))
        in_items.append(merged)
        in_pos.append(ptr[-1] + np.searchsorted(merged, dec))
        ptr.append(ptr[-1] + len(dec))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return {"users": np.asarray(users, np.int64), "entry_ptr": np.asarray(ptr, np.int64), "items": cat(items, np.int64),
            "labels": cat(labels, np.float64), "slot": cat(slot, np.int64), "in_items": cat(in_items, np.int64),
            "in_pos": cat(in_pos, np.int64)}


# ---------------------------------------------------------------------------------------------- the graph
def _act(z, act):
    return z if act == "identity" else 1.0 / (1.0 + np.exp(-z))


def encode(T, in_slot, in_items, keep, keep_prob, users, act, dt):
    one = dt(1.0)
    val = np.asarray(keep, dt) * (one / dt(keep_prob))
    B, d = len(users), T["en_embeddings"].shape[1]
    pooled = np.zeros((B, d), dt)
    for e in range(len(in_items)):                          # entry order, as sparse_tensor_dense_matmul walks it
        if val[e] != 0:
            pooled[in_slot[e]] += val[e] * T["en_embeddings"][in_items[e]]
    return _act((pooled + T["user_embeddings"][users]) + T["en_offset"], act).astype(dt)


def loss_terms(T, batch, keep, keep_prob, reg, act, loss, dtype=np.float64):
    """(data term, regulariser term, cache)"""
    dt = dtype
    T = {k: np.asarray(v, dt) for k, v in T.items()}
    users, items, slot = batch["users"], batch["items"], batch["slot"]
    ptr = batch["entry_ptr"]
    in_slot = np.repeat(np.arange(len(users)), np.diff(ptr))
    hidden = encode(T, in_slot, batch["in_items"], keep, keep_prob, users, act, dt)
    x = np.einsum("ed,ed->e", hidden[slot], T["de_embeddings"][items]).astype(dt) + T["de_bias"][items]
    z = np.asarray(batch["labels"], dt)
    if loss == "square":
        per = (x - z) ** 2
        g = 2 * (x - z)
    else:
        per = np.maximum(x, 0) - x * z + np.log1p(np.exp(-np.abs(x)))
        g = 1.0 / (1.0 + np.exp(-x)) - z
    uniq = np.unique(items)
    l2 = 0.5 * ((T["en_embeddings"][uniq] ** 2).sum() + (T["de_embeddings"][uniq] ** 2).sum() +
                (T["de_bias"][uniq] ** 2).sum() + (T["user_embeddings"][users] ** 2).sum() + (T["en_offset"] ** 2).sum())
    return dt(per.sum(dtype=dt)), dt(dt(reg) * l2), (T, hidden, g.astype(dt), in_slot, uniq)


def gradients(T, batch, keep, keep_prob, reg, act, loss, dtype=np.float64):
    """((data term, regulariser term), {name: gradient}) of the summed loss"""
    dt = dtype
    data, regul, (T, hidden, g, in_slot, uniq) = loss_terms(T, batch, keep, keep_prob, reg, act, loss, dt)
    users, items, slot = batch["users"], batch["items"], batch["slot"]
    G = {k: np.zeros_like(v) for k, v in T.items()}
    dh = np.zeros_like(hidden)
    for e in range(len(items)):
        G["de_embeddings"][items[e]] += g[e] * hidden[slot[e]]
        G["de_bias"][items[e]] += g[e]
        dh[slot[e]] += g[e] * T["de_embeddings"][items[e]]
    dz = dh if act == "identity" else dh * (hidden * (1 - hidden))
    val = np.asarray(keep, dt) * (dt(1.0) / dt(keep_prob))
    for e in range(len(batch["in_items"])):
        if val[e] != 0:
            G["en_embeddings"][batch["in_items"][e]] += val[e] * dz[in_slot[e]]
    for s, u in enumerate(users):
        G["user_embeddings"][u] += dz[s]
    G["en_offset"] += dz.sum(axis=0)
    r = dt(reg)
    for k in ("en_embeddings", "de_embeddings", "de_bias"):
        G[k][uniq] += r * T[k][uniq]
    for u in users:
        G["user_embeddings"][u] += r * T["user_embeddings"][u]
    G["en_offset"] += r * T["en_offset"]
    return (data, regul), G


def predict(T, indptr, indices, users, keep, keep_prob, act, dtype=np.float64):
    """CDAE.py:148-160: [B, I] from the users' train rows, corrupted by `keep` (one flag per train entry, in order)"""
    dt = dtype
    T = {k: np.asarray(v, dt) for k, v in T.items()}
    deg = [indptr[u + 1] - indptr[u] for u in users]
    in_slot = np.repeat(np.arange(len(users)), deg)
    in_items = np.concatenate([indices[indptr[u]:indptr[u + 1]] for u in users]).astype(np.int64) if len(users) \
        else np.zeros(0, np.int64)
    hidden = encode(T, in_slot, in_items, keep, keep_prob, np.asarray(users, np.int64), act, dt)
    return hidden @ T["de_embeddings"].T + T["de_bias"], hidden


class Adam:
    """tf.train.AdamOptimizer(lr) as TF-1.12 applies it here: the sparse form on the four row tables (every row's
    moments decay every step), ApplyAdam on en_offset — the same update in exact arithmetic"""

    def __init__(self, T, lr, dtype=np.float64):
        self.dt, self.lr, self.t = dtype, dtype(lr), 0
        self.T = {k: np.asarray(v, dtype).copy() for k, v in T.items()}
        self.m = {k: np.zeros_like(v) for k, v in self.T.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.T.items()}

    def apply(self, G):
        dt = self.dt
        self.t += 1
        b1, b2, eps = dt(0.9), dt(0.999), dt(1e-8)
        alpha = self.lr * np.sqrt(dt(1) - b2 ** self.t) / (dt(1) - b1 ** self.t)
        for k in self.T:
            g = np.asarray(G[k], dt)
            self.m[k] = self.m[k] * b1 + g * (dt(1) - b1)
            self.v[k] = self.v[k] * b2 + (g * g) * (dt(1) - b2)
            self.T[k] = self.T[k] - alpha * self.m[k] / (np.sqrt(self.v[k]) + eps)
