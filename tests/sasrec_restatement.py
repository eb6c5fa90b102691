"""SASRec restated in numpy from model/sequential_recommender/SASRec.py of the reference: forward, hand-derived
backward and the Adam forms, in float32 or float64.

One routine, `row_pass`, runs a single sequence over a WINDOW [w0, L) of its positions with every mask of the reference
written out (key mask from sum(keys) == 0, causal mask, query mask from sum(q) == 0, the row mask, is_target):

  * `form="mask"`    w0 = 0: the reference's full form, padded rows computed like any other row;
  * `form="suffix"`  w0 = the first real position: only the row's real suffix is computed.  Padded positions enter in
                     one place only: a query none of whose keys is visible gets the reference's uniform softmax over all
                     L keys (every logit is -2**32 + 1), and the w0 padded keys carry V = bv there.

tests/test_sasrec_cpu.py asserts that the two forms agree and checks both against the trace of the reference class.

Variables in creation order (SASRec.py:299-356): item_emb [I, d], pos_emb [L, d]; per block i: b<i>_ln1_beta,
b<i>_ln1_gamma, b<i>_Wq, b<i>_bq, b<i>_Wk, b<i>_bk, b<i>_Wv, b<i>_bv, b<i>_ln2_beta, b<i>_ln2_gamma, b<i>_W1 (conv1d
kernel [1, d, d] kept as [d, d]), b<i>_b1, b<i>_W2, b<i>_b2; then lnf_beta, lnf_gamma.
Dropout sites in evaluation order: the embedding [B, L, d]; per block the attention weights [h B, L, L] (head-major),
the feed-forward's hidden [B, L, d] and its output [B, L, d].
"""
import numpy as np

LR = 0.001
BETA1, BETA2, EPS = 0.9, 0.98, 1e-8
LN_EPS = 1e-8
LOG_EPS = 1e-24
# case -> (hidden_units, num_heads, num_blocks, max_len, l2_emb, dropout_rate)
CASES = {"first": (12, 1, 2, 7, 0.0, 0.0), "second": (8, 2, 1, 5, 0.01, 0.5), "third": (50, 1, 2, 10, 0.0, 0.5)}
PREDICT_CASE = "third"
_BLOCK = ("ln1_beta", "ln1_gamma", "Wq", "bq", "Wk", "bk", "Wv", "bv", "ln2_beta", "ln2_gamma", "W1", "b1", "W2", "b2")


def numpy_batch_randint_choice(high, size, replace=True, p=None, exclusion=None):
    """`batch_randint_choice` over numpy's global stream, for the traces and the CPU tests (the reference draws from
    glibc rand(), the package from the device sampler): per request, draws of the missing count until none is
    excluded.  Always a list per request, an empty one for size 0."""
    assert replace and p is None
    out = []
    for idx, n in enumerate(size):
        exc = set(int(e) for e in exclusion[idx]) if exclusion is not None else set()
        got = []
        while len(got) < n:
            got += [int(a) for a in np.random.randint(0, high, size=n - len(got)) if int(a) not in exc]
        out.append(got)
    return out


def table_names(num_blocks):
    out = ["item_emb", "pos_emb"]
    for i in range(num_blocks):
        out += ["b%d_%s" % (i, n) for n in _BLOCK]
    return out + ["lnf_beta", "lnf_gamma"]


def init_tables(n_items, d, max_len, num_blocks, seed):
    """small random values for every variable, the layer-norm offsets included (a zero beta hides the padded rows).
    item_emb rows have a norm near 2 / sqrt(d): the looked-up table is sqrt(d) times that and meets layer-normed rows of
    norm sqrt(d), so the logits are O(2) and no sigmoid saturates (a saturated one differs between the float widths by
    design; the GPU tests have a case of their own for those)."""
    rs = np.random.RandomState(seed)
    t = {"item_emb": rs.randn(n_items, d) * (2.0 / d), "pos_emb": rs.randn(max_len, d) * 0.3}
    for i in range(num_blocks):
        for n in _BLOCK:
            if n.startswith("W"):
                v = rs.randn(d, d) * (0.6 / np.sqrt(d))
            elif n.endswith("gamma"):
                v = 1.0 + rs.randn(d) * 0.1
            else:
                v = rs.randn(d) * 0.1
            t["b%d_%s" % (i, n)] = v
    t["lnf_beta"], t["lnf_gamma"] = rs.randn(d) * 0.1, 1.0 + rs.randn(d) * 0.1
    return {k: v.astype(np.float32) for k, v in t.items()}


def n_sites(num_blocks):
    return 1 + 3 * num_blocks


def site_shapes(B, L, d, h, num_blocks):
    out = [(B, L, d)]
    for _ in range(num_blocks):
        out += [(h * B, L, L), (B, L, d), (B, L, d)]
    return out


def _ln(x, beta, gamma):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)                  # tf.nn.moments: the biased variance
    rstd = 1.0 / np.sqrt(var + x.dtype.type(LN_EPS))
    xh = (x - mu) * rstd
    return gamma * xh + beta, xh, rstd


def _ln_bwd(dy, xh, rstd, gamma, G, kb, kg):
    G[kg] += (dy * xh).sum(0)
    G[kb] += dy.sum(0)
    dxh = dy * gamma
    return rstd * (dxh - dxh.mean(-1, keepdims=True) - xh * (dxh * xh).mean(-1, keepdims=True))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def row_pass(T, seq, pos, neg, n_items, h, rate, masks, b, B, w0, inv_T=None, G=None, training=True):
    """One sequence over the window [w0, L).  T: {name: array} in the working width; masks: the dropout sites' {0, 1}
    arrays (None: rate 0 or evaluation), b: this row's index in them.  With G (gradient accumulators) and inv_T
    (1 / sum(is_target) of the batch) the backward pass runs too.  Returns (sum of the row's loss terms, z [L - w0, d])."""
    dt = T["item_emb"].dtype
    L, d = T["pos_emb"].shape
    nb = (len(T) - 4) // len(_BLOCK)
    dh = d // h
    I = n_items
    m = L - w0
    keep = dt.type(1.0) / (dt.type(1.0) - dt.type(rate)) if (training and rate) else dt.type(1.0)
    use = training and masks is not None
    site = lambda k: masks[k].astype(dt) if use else None
    sd = dt.type(d) ** dt.type(0.5)
    table = np.concatenate([T["item_emb"], np.zeros((1, d), dt)]) * sd
    s, p_, n_ = seq[w0:], pos[w0:], neg[w0:]
    rowmask = (s != I).astype(dt)[:, None]
    x = table[s] + T["pos_emb"][w0:]
    dm0 = site(0)[b, w0:] if use else None
    if use:
        x = x * dm0 * keep
    x = x * rowmask
    saved = []
    tril = np.tril(np.ones((m, m), bool))
    for i in range(nb):
        P = lambda n: T["b%d_%s" % (i, n)]
        q, xh1, rstd1 = _ln(x, P("ln1_beta"), P("ln1_gamma"))
        Q, K, V = q @ P("Wq") + P("bq"), x @ P("Wk") + P("bk"), x @ P("Wv") + P("bv")
        kvis = x.sum(-1) != 0
        qm = (q.sum(-1) != 0).astype(dt)[:, None]
        allowed = tril & kvis[None, :]
        anyv = allowed.any(1)
        O = np.zeros((m, d), dt)
        heads = []
        for hd in range(h):
            sl = slice(hd * dh, (hd + 1) * dh)
            S = (Q[:, sl] @ K[:, sl].T) / (dt.type(dh) ** dt.type(0.5))
            Sm = np.where(allowed, S, -np.inf)
            mx = np.where(anyv, Sm.max(1, initial=-np.inf), 0)[:, None]
            Ex = np.where(allowed, np.exp(np.where(allowed, S - mx, 0)), 0).astype(dt)
            den = np.where(anyv, Ex.sum(1), 1)[:, None]
            Pw = np.where(anyv[:, None], Ex / den, dt.type(1.0) / dt.type(L)).astype(dt)   # no visible key: uniform over L
            dmA = site(1 + 3 * i)[hd * B + b] if use else None
            W = Pw * qm
            if use:
                W = W * dmA[w0:, w0:] * keep
            O[:, sl] = W @ V[:, sl]
            padw = None
            if w0:                                         # the w0 padded keys of a uniform row: V = bv
                padw = np.where(anyv, 0, dt.type(1.0) / dt.type(L)).astype(dt)[:, None] * qm
                padw = padw * ((dmA[w0:, :w0].sum(1, keepdims=True) * keep) if use else dt.type(w0))
                O[:, sl] += padw * P("bv")[sl]
            heads.append((Pw, W, padw, dmA))
        y = O + q
        u, yh, rstd2 = _ln(y, P("ln2_beta"), P("ln2_gamma"))
        h1 = u @ P("W1") + P("b1")
        a = np.maximum(h1, 0)
        dm1, dm2 = (site(2 + 3 * i)[b, w0:], site(3 + 3 * i)[b, w0:]) if use else (None, None)
        if use:
            a = a * dm1 * keep
        f = a @ P("W2") + P("b2")
        if use:
            f = f * dm2 * keep
        saved.append(dict(x=x, q=q, xh1=xh1, rstd1=rstd1, Q=Q, K=K, V=V, qm=qm, anyv=anyv, heads=heads, yh=yh,
                          rstd2=rstd2, u=u, h1=h1, a=a, dm1=dm1, dm2=dm2))
        x = (f + u) * rowmask
    z, zh, rstdf = _ln(x, T["lnf_beta"], T["lnf_gamma"])
    tp, tn = table[p_], table[n_]
    lp, ln_ = (tp * z).sum(-1), (tn * z).sum(-1)
    it = (p_ != I).astype(dt)
    sp, sn = _sigmoid(lp), _sigmoid(ln_)
    one, le = dt.type(1.0), dt.type(LOG_EPS)
    with np.errstate(divide="ignore"):
        terms = (-np.log(sp + le) - np.log(one - sn + le)) * it
    loss_sum = terms.sum()
    if G is None:
        return loss_sum, z
    # ---------------------------------------------------------------- backward
    dp = -(sp * (one - sp)) / (sp + le) * it * inv_T
    dn = (sn * (one - sn)) / (one - sn + le) * it * inv_T
    dz = dp[:, None] * tp + dn[:, None] * tn
    for ids, dl in ((p_, dp), (n_, dn)):
        real = ids != I
        np.add.at(G["item_emb"], ids[real], (dl[:, None] * z * sd)[real])
    dx = _ln_bwd(dz, zh, rstdf, T["lnf_gamma"], G, "lnf_beta", "lnf_gamma")
    for i in reversed(range(nb)):
        P = lambda n: T["b%d_%s" % (i, n)]
        g = lambda n: "b%d_%s" % (i, n)
        c = saved[i]
        dfu = dx * rowmask
        df = dfu * c["dm2"] * keep if use else dfu
        G[g("W2")] += c["a"].T @ df
        G[g("b2")] += df.sum(0)
        da = df @ P("W2").T
        if use:
            da = da * c["dm1"] * keep
        dh1 = da * (c["h1"] > 0)
        G[g("W1")] += c["u"].T @ dh1
        G[g("b1")] += dh1.sum(0)
        du = dfu + dh1 @ P("W1").T
        dy = _ln_bwd(du, c["yh"], c["rstd2"], P("ln2_gamma"), G, g("ln2_beta"), g("ln2_gamma"))
        dq = dy.copy()
        dQ, dK, dV = np.zeros((m, d), dt), np.zeros((m, d), dt), np.zeros((m, d), dt)
        for hd in range(h):
            sl = slice(hd * dh, (hd + 1) * dh)
            Pw, W, padw, dmA = c["heads"][hd]
            dO = dy[:, sl]
            dV[:, sl] = W.T @ dO
            if padw is not None:
                G[g("bv")][sl] += (padw * dO).sum(0)
            dW = dO @ c["V"][:, sl].T
            dP = dW * c["qm"]
            if use:
                dP = dP * dmA[w0:, w0:] * keep
            dS = Pw * (dP - (dP * Pw).sum(1, keepdims=True))
            dS = np.where(c["anyv"][:, None], dS, 0) / (dt.type(dh) ** dt.type(0.5))
            dQ[:, sl] = dS @ c["K"][:, sl]
            dK[:, sl] = dS.T @ c["Q"][:, sl]
        for nm, src, dd in (("q", c["q"], dQ), ("k", c["x"], dK), ("v", c["x"], dV)):
            G[g("W" + nm)] += src.T @ dd
            G[g("b" + nm)] += dd.sum(0)
        dq += dQ @ P("Wq").T
        dx = dK @ P("Wk").T + dV @ P("Wv").T
        dx += _ln_bwd(dq, c["xh1"], c["rstd1"], P("ln1_gamma"), G, g("ln1_beta"), g("ln1_gamma"))
    de = dx * rowmask
    if use:
        de = de * dm0 * keep
    G["pos_emb"][w0:] += de
    real = s != I
    np.add.at(G["item_emb"], s[real], (de * sd)[real])
    return loss_sum, z


def first_real(seq_row, n_items):
    real = np.flatnonzero(seq_row != n_items)
    return int(real[0]) if len(real) else len(seq_row)


def gradients(tables, seq, pos, neg, n_items, h, rate, l2_emb, masks=None, form="suffix", dtype=np.float64):
    """(loss, {name: gradient}) of one batch; the loss holds the regulariser when l2_emb != 0 (SASRec.py:377-381)"""
    T = {k: np.asarray(v, dtype) for k, v in tables.items()}
    G = {k: np.zeros_like(v) for k, v in T.items()}
    B, L = seq.shape
    n_target = int((pos != n_items).sum())
    inv_T = dtype(1.0) / dtype(n_target)
    total = dtype(0.0)
    for b in range(B):
        w0 = first_real(seq[b], n_items) if form == "suffix" else 0
        if form == "suffix":
            assert (pos[b, :w0] == n_items).all(), "a target at a padded position"
            if w0 == L:
                continue
        ls, _ = row_pass(T, seq[b], pos[b], neg[b], n_items, h, rate, masks, b, B, w0, inv_T, G)
        total += ls
    loss = total * inv_T
    if l2_emb:
        for k in ("item_emb", "pos_emb"):
            loss += dtype(l2_emb) * (T[k] ** 2).sum() / 2
            G[k] += dtype(l2_emb) * T[k]
    return loss, G


def final_rows(tables, seq, n_items, h, form="suffix", dtype=np.float64):
    """seq[:, -1, :] with training off (predict's user embeddings)"""
    T = {k: np.asarray(v, dtype) for k, v in tables.items()}
    B, L = seq.shape
    out = np.zeros((B, T["pos_emb"].shape[1]), dtype)
    pad = np.full(L, n_items, seq.dtype)
    for b in range(B):
        w0 = first_real(seq[b], n_items) if form == "suffix" else 0
        if w0 == L:
            out[b] = T["lnf_beta"]                       # the all-padded row normalises to beta
            continue
        _, z = row_pass(T, seq[b], pad, pad, n_items, h, 0.0, None, b, B, w0, training=False)
        out[b] = z[-1]
    return out


def scores(tables, seq, n_items, h, form="suffix", dtype=np.float64):
    T = np.asarray(tables["item_emb"], dtype)
    d = T.shape[1]
    return final_rows(tables, seq, n_items, h, form, dtype) @ (T * dtype(d) ** dtype(0.5)).T


class Adam:
    """TF-1.12's Adam as the optimiser picks its forms for this graph: pos_emb in the sparse form when it has no
    regulariser (its only consumer is then a gather), everything else ApplyAdam"""

    def __init__(self, tables, l2_emb, dtype=np.float64, lr=LR, beta2=BETA2):
        self.dt = dtype
        self.m = {k: np.zeros(np.shape(v), dtype) for k, v in tables.items()}
        self.v = {k: np.zeros(np.shape(v), dtype) for k, v in tables.items()}
        self.lr, self.b1, self.b2, self.eps = dtype(lr), dtype(BETA1), dtype(beta2), dtype(EPS)
        self.b1p, self.b2p = self.b1, self.b2
        self.sparse = {"pos_emb"} if not l2_emb else set()

    def apply(self, T, G):
        one = self.dt(1.0)
        alpha = self.lr * np.sqrt(one - self.b2p) / (one - self.b1p)
        for k in T:
            m, v, g = self.m[k], self.v[k], G[k]
            if k in self.sparse:
                m[...] = m * self.b1 + g * (one - self.b1)
                v[...] = v * self.b2 + (g * g) * (one - self.b2)
                T[k] = T[k] - alpha * m / (np.sqrt(v) + self.eps)
            else:
                m += (g - m) * (one - self.b1)
                v += (g * g - v) * (one - self.b2)
                T[k] = T[k] - (m * alpha) / (np.sqrt(v) + self.eps)
        self.b1p, self.b2p = self.b1p * self.b1, self.b2p * self.b2


def train(tables, feeds, n_items, h, rate, l2_emb, masks_per_step=None, form="suffix", dtype=np.float64):
    """the tables after each step of `feeds` [(seq, pos, neg)], and the losses before each update"""
    T = {k: np.asarray(v, dtype) for k, v in tables.items()}
    opt = Adam(T, l2_emb, dtype)
    out, losses = [], []
    for s, (seq, pos, neg) in enumerate(feeds):
        if int((pos != n_items).sum()) == 0:
            out.append({k: v.copy() for k, v in T.items()})
            losses.append(dtype(0.0))
            continue
        loss, G = gradients(T, seq, pos, neg, n_items, h, rate, l2_emb,
                            None if masks_per_step is None else masks_per_step[s], form, dtype)
        opt.apply(T, G)
        out.append({k: v.copy() for k, v in T.items()})
        losses.append(loss)
    return out, losses
