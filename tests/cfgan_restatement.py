"""CFGAN restated in numpy: the graph of CFGAN.py:53-95 with its gradients, the two optimisers (TF-1.12 ApplyAdam /
gradient descent, each over its own variable list), the scorer, and — bit for bit — the device's mask builder
(csrc/cfgan.hip: mask_base / mask_pair and the n smallest (key, column) pairs).  float64 unless a dtype is asked for."""
import numpy as np

U64 = np.uint64

# the cases of tests/golden/tfgraph_cfgan.npz:
#   (mode, hiddenLayer_G, hiddenLayer_D, reg_G, reg_D, opt_G, opt_D, step_D, step_G)
CASES = {"user": ("userBased", [24], [10], 0.001, 0.0, "adam", "adam", 1, 1),
         "item": ("itemBased", [24], [10], 0.001, 0.01, "adam", "adam", 1, 1),
         "deep": ("userBased", [24, 12], [10, 6], 0.001, 0.0, "sgd", "adam", 1, 1),
         "steps": ("userBased", [24], [10], 0.001, 0.0, "adam", "adam", 2, 2)}
EPOCH_CASE = "user"
LR_G, LR_D, ZR_RATIO, ZP_RATIO, ZR_COEF, BATCH_G, BATCH_D = 0.001, 0.002, 0.7, 0.5, 0.03, 14, 16


# ---------------------------------------------------------------------------------------------- names and shapes
def names(n_g, n_d):
    """the variables in the reference's creation order (CFGAN.py:97-123)"""
    out = []
    for net, n in (("gen", n_g), ("dis", n_d)):
        for k in range(n):
            out += ["%s_h%d_kernel" % (net, k), "%s_h%d_bias" % (net, k)]
        out += ["%s_out_kernel" % net, "%s_out_bias" % net]
    return out


def shapes(n_cols, hidden_g, hidden_d):
    out = {}
    for net, widths, n_in, n_out in (("gen", hidden_g, n_cols, n_cols), ("dis", hidden_d, 2 * n_cols, 1)):
        for k, w in enumerate(widths):
            out["%s_h%d_kernel" % (net, k)] = (n_in, int(w))
            out["%s_h%d_bias" % (net, k)] = (int(w),)
            n_in = int(w)
        out["%s_out_kernel" % net] = (n_in, n_out)
        out["%s_out_bias" % net] = (n_out,)
    return out


def init_tables(n_cols, hidden_g, hidden_d, seed):
    """Xavier-uniform kernels, zero biases, float32, drawn in creation order from one stream"""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in shapes(n_cols, hidden_g, hidden_d).items():
        if len(shape) == 2:
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            out[name] = rs.uniform(-lim, lim, shape).astype(np.float32)
        else:
            out[name] = np.zeros(shape, np.float32)
    return out


def layers_of(tables, net):
    """[(kernel, bias)] of a network, hidden layers first"""
    out, k = [], 0
    while "%s_h%d_kernel" % (net, k) in tables:
        out.append((tables["%s_h%d_kernel" % (net, k)], tables["%s_h%d_bias" % (net, k)]))
        k += 1
    return out + [(tables["%s_out_kernel" % net], tables["%s_out_bias" % net])]


def layer_names(tables, net):
    n = len(layers_of(tables, net)) - 1
    return [("%s_h%d_kernel" % (net, k), "%s_h%d_bias" % (net, k)) for k in range(n)] + \
        [("%s_out_kernel" % net, "%s_out_bias" % net)]


# ---------------------------------------------------------------------------------------------- the masks
def splitmix64(x):
    """nr::splitmix64 on uint64 arrays"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, U64) + U64(0x9e3779b97f4a7c15)
        x = (x ^ (x >> U64(30))) * U64(0xbf58476d1ce4e5b9)
        x = (x ^ (x >> U64(27))) * U64(0x94d049bb133111eb)
        return x ^ (x >> U64(31))


def mask_base(seed, epoch, plane, row):
    with np.errstate(over="ignore"):
        e = np.asarray([int(epoch) & 0xffffffffffffffff], U64) * U64(0xd1342543de82ef95) + U64(0x632be59bd9b4e019)
        z = splitmix64(np.asarray([int(seed) & 0xffffffffffffffff], U64) ^ splitmix64(e))
        return splitmix64(z ^ U64((int(row) << 1) | (int(plane) & 1)))


def column_keys(seed, epoch, plane, row, n_cols):
    """the 32-bit key of every column"""
    with np.errstate(over="ignore"):
        return (splitmix64(mask_base(seed, epoch, plane, row) + np.arange(n_cols, dtype=U64)) >> U64(32)).astype(np.int64)


def n_sample(n_cols, deg, ratio):
    """CFGAN.py:141,145 in Python doubles; a row without a train entry is not in user_pos_train and gets no sample"""
    return int((n_cols - deg) * ratio) if deg > 0 else 0


def mask_row(pos_cols, n_cols, n, seed, epoch, plane, row):
    """bool [n_cols]: the positives and the n other columns with the smallest (key, column) pairs"""
    have = np.zeros(n_cols, bool)
    have[np.asarray(pos_cols, np.int64)] = True
    free = np.flatnonzero(~have)
    n = min(max(int(n), 0), len(free))
    if n:
        keys = column_keys(seed, epoch, plane, row, n_cols)[free]
        have[free[np.lexsort((free, keys))[:n]]] = True
    return have


def to_bits(dense):
    """bool / 0-1 [B, n_cols] -> uint32 [B, ceil(n_cols / 32)], column 32 w + k at bit k of word w"""
    dense = np.atleast_2d(np.asarray(dense) != 0)
    B, n = dense.shape
    words = (n + 31) // 32
    pad = np.zeros((B, words * 32), np.uint8)
    pad[:, :n] = dense
    return np.packbits(pad, axis=1, bitorder="little").view("<u4").reshape(B, words).astype(np.uint32)


def from_bits(bits, n_cols):
    bits = np.ascontiguousarray(np.atleast_2d(bits).astype("<u4"))
    return np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :n_cols].astype(bool)


def masks(indptr, indices, rows, counts, n_cols, seed, epoch):
    """(zr, pm) bit rows of the batch `rows`; counts [B, 2]: the sample sizes per row and plane"""
    out = []
    for plane in (0, 1):
        dense = [mask_row(indices[indptr[r]:indptr[r + 1]], n_cols, counts[b][plane], seed, epoch, plane, r)
                 for b, r in enumerate(rows)]
        out.append(to_bits(np.stack(dense)) if len(dense) else np.zeros((0, (n_cols + 31) // 32), np.uint32))
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------- the graph
def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def cross_entropy(label, x):
    """tf.nn.sigmoid_cross_entropy_with_logits"""
    return np.maximum(x, 0) - x * label + np.log1p(np.exp(-np.abs(x)))


def mlp_forward(x, layers):
    """[input, hidden activations ..., output]"""
    acts = [x]
    for k, (W, b) in enumerate(layers):
        z = acts[-1] @ W + b
        acts.append(z if k == len(layers) - 1 else sigmoid(z))
    return acts


def mlp_backward(acts, d_out, layers):
    """([(dW, db)] per layer, d input) from the derivative at the output"""
    grads, d = [None] * len(layers), d_out
    for k in range(len(layers) - 1, -1, -1):
        if k < len(layers) - 1:
            d = d * acts[k + 1] * (1.0 - acts[k + 1])
        grads[k] = (acts[k].T @ d, d.sum(0))
        d = d @ layers[k][0].T
    return grads, d


class Optimizer:
    """one tf.train optimiser object over its own variables: ApplyAdam with its own beta powers, or gradient descent"""

    def __init__(self, kind, lr, dtype):
        self.kind, self.dt = kind, dtype
        self.lr, self.b1, self.b2, self.eps = (dtype(x) for x in (lr, 0.9, 0.999, 1e-8))
        self.b1p, self.b2p, self.slots, self.t = self.b1, self.b2, {}, 0

    def apply(self, tables, grads):
        one = self.dt(1.0)
        for name, g in grads.items():
            var = tables[name]
            if self.kind == "sgd":
                tables[name] = var - self.lr * g
                continue
            m, v = self.slots.setdefault(name, (np.zeros_like(var), np.zeros_like(var)))
            alpha = self.lr * np.sqrt(one - self.b2p) / (one - self.b1p)
            m += (g - m) * (one - self.b1)
            v += (g * g - v) * (one - self.b2)
            tables[name] = var - (m * alpha) / (np.sqrt(v) + self.eps)
        if self.kind == "adam":
            self.b1p, self.b2p = self.b1p * self.b1, self.b2p * self.b2
        self.t += 1


class CFGAN:
    """R: scipy CSR whose rows are the model's rows (already transposed for itemBased)"""

    def __init__(self, tables, R, lr_G, lr_D, reg_G, reg_D, zr_coef, opt_G="adam", opt_D="adam", dtype=np.float64):
        self.dt = dtype
        self.T = {k: np.asarray(v).astype(dtype) for k, v in tables.items()}
        self.R = R.tocsr()
        self.n_rows, self.n_cols = self.R.shape
        self.reg_G, self.reg_D, self.zr_coef = dtype(reg_G), dtype(reg_D), dtype(zr_coef)
        self.opt_G, self.opt_D = Optimizer(opt_G, lr_G, dtype), Optimizer(opt_D, lr_D, dtype)

    def rows(self, rows):
        return np.asarray(self.R[np.asarray(rows, np.int64)].todense()).astype(self.dt) if len(rows) else \
            np.zeros((0, self.n_cols), self.dt)

    def _forward(self, rows, pm):
        c = self.rows(rows)
        g_acts = mlp_forward(c, layers_of(self.T, "gen"))
        y = g_acts[-1] * pm
        return c, g_acts, y

    def _reg(self, net, reg):
        return reg * sum((v * v).sum() for k, v in self.T.items() if k.startswith(net)) / 2

    def d_gradients(self, rows, zr, pm):
        """((real, fake, regulariser) loss terms, {name: gradient}) of trainer_d's loss"""
        B, n = len(rows), self.n_cols
        pm = np.asarray(pm, self.dt)
        c, _, y = self._forward(rows, pm)
        D = layers_of(self.T, "dis")
        acts = mlp_forward(np.concatenate([np.concatenate([c, c], 1), np.concatenate([c, y], 1)], 0), D)
        logit = acts[-1]
        real, fake = cross_entropy(1.0, logit[:B]).mean(), cross_entropy(0.0, logit[B:]).mean()
        d = np.concatenate([sigmoid(logit[:B]) - 1.0, sigmoid(logit[B:])], 0) / B
        grads, _ = mlp_backward(acts, d.astype(self.dt), D)
        out = {}
        for (kn, bn), (dW, db) in zip(layer_names(self.T, "dis"), grads):
            out[kn], out[bn] = dW + self.reg_D * self.T[kn], db + self.reg_D * self.T[bn]
        return (real, fake, self._reg("dis", self.reg_D)), out

    def g_gradients(self, rows, zr, pm):
        """((adversarial, regulariser, zero-reconstruction) loss terms, {name: gradient}) of trainer_g's loss"""
        B, n = len(rows), self.n_cols
        zr, pm = np.asarray(zr, self.dt), np.asarray(pm, self.dt)
        c, g_acts, y = self._forward(rows, pm)
        D, G = layers_of(self.T, "dis"), layers_of(self.T, "gen")
        acts = mlp_forward(np.concatenate([c, y], 1), D)
        logit, out = acts[-1], g_acts[-1]
        adv = cross_entropy(1.0, logit).mean()
        zr_loss = self.zr_coef * (out * out * zr).sum(1).mean()
        _, dx = mlp_backward(acts, ((sigmoid(logit) - 1.0) / B).astype(self.dt), D)
        d_out = dx[:, n:] * pm + (2 * self.zr_coef / B) * out * zr
        grads, _ = mlp_backward(g_acts, d_out.astype(self.dt), G)
        res = {}
        for (kn, bn), (dW, db) in zip(layer_names(self.T, "gen"), grads):
            res[kn], res[bn] = dW + self.reg_G * self.T[kn], db + self.reg_G * self.T[bn]
        return (adv, self._reg("gen", self.reg_G), zr_loss), res

    def d_step(self, rows, zr, pm):
        if len(rows) == 0:
            return None
        loss, grads = self.d_gradients(rows, zr, pm)
        self.opt_D.apply(self.T, grads)
        return loss

    def g_step(self, rows, zr, pm):
        if len(rows) == 0:
            return None
        loss, grads = self.g_gradients(rows, zr, pm)
        self.opt_G.apply(self.T, grads)
        return loss

    def ratings(self, rows=None):
        """G(R) for `rows` (None: every row)"""
        rows = np.arange(self.n_rows) if rows is None else rows
        return mlp_forward(self.rows(rows), layers_of(self.T, "gen"))[-1]
