"""A restatement of NAIS (NAIS.py:96-176, util/learner.py, TF-1.12's optimiser kernels) for the NAIS tests: one training
step on the PADDED form with torch autograd (float64 by default), independent of the derivation in csrc/nais.hip, and
predict().  Both mask forms: "reference" = sequence_mask(|H| + 1) cut at the side's longest history (one zero row
inside the mask of every shorter instance), "history" = exactly H.  Checked against the reference class's own f64 trace
in test_nais_cpu.py; the GPU tests use it for the shapes the trace does not hold.  The instance rule and the learners
are fism_restatement's."""
import numpy as np
import torch

import fism_restatement as F

NAMES = ("c1", "Q", "bias", "W", "b", "h")


def load_trace(load_golden):
    """the two fixture files as one mapping (the case with the 1,100-item history has a file of its own)"""
    g = dict(load_golden("tfgraph_nais"))
    g.update(load_golden("tfgraph_nais_long"))
    return g


def golden_tables(g, case, tag, step):
    """(c1, Q, bias, W, b, h) of the trace after `step` (0-based), in the trace's width"""
    dt = np.float32 if tag == "f32" else np.float64
    alg = int(g[case + "_hyper"][0])
    out = F.golden_tables(g, case, tag, step)
    for name, init in (("W", g["W0_a%d" % alg]), ("b", g["b_0"]), ("h", g["h_0"])):
        out.append((init.astype(np.float64) + g["%s_%s_%s" % (case, tag, name)][step]).astype(dt))
    return out


def golden_hyper(g, case):
    alg, act, alpha, beta = g[case + "_hyper"]
    return dict(algorithm=int(alg), activation=int(act), alpha=float(alpha), beta=float(beta))


class State(F.State):
    def __init__(self, c1, Q, bias, W, b, h, learner="adam", lr=0.01, momentum=0.9, dtype=np.float64):
        F.State.__init__(self, c1, Q, bias, learner=learner, lr=lr, momentum=momentum)
        for k, v in (("W", W), ("b", np.reshape(b, -1)), ("h", np.reshape(h, -1))):
            self.var[k] = np.array(v, dtype=np.float64)
        init = {"adam": 0.0, "gd": 0.0, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        if dtype != np.float64:
            self.var = {k: v.astype(dtype) for k, v in self.var.items()}
        self.s0 = {k: np.full_like(v, init) for k, v in self.var.items()}
        self.s1 = {k: np.zeros_like(v) for k, v in self.var.items()}


def _act(z, activation):
    if activation == 0:
        return torch.relu(z)
    if activation == 1:
        return torch.sigmoid(z)
    if activation == 2:
        return torch.tanh(z)
    return z


def _side(T, ids, width_mask, item, n, algorithm, activation, alpha, beta):
    """_create_inference on one padded side: ids [B, L] (pad = num_items), width_mask [B, L]"""
    c1, Q, bias, W, b, h = T
    table = torch.cat([c1, torch.zeros(1, c1.shape[1], dtype=c1.dtype)], dim=0)
    e_ = table[ids]                                            # (B, L, d)
    q = Q[item]                                                # (B, d)
    x = e_ * q[:, None, :] if algorithm == 0 else torch.cat([e_, q[:, None, :].expand(-1, e_.shape[1], -1)], dim=2)
    a = _act(x @ W + b[None, None, :], activation)
    ex = torch.exp(a @ h) * width_mask
    S = ex.sum(dim=1, keepdim=True)
    S = torch.where(S > 0, S, torch.ones_like(S)) ** beta      # an empty mask ("history" form): p = 0
    p = ((ex / S)[:, :, None] * e_).sum(dim=1) if ids.shape[1] else torch.zeros_like(q)
    out = n ** alpha * (p * q).sum(dim=1) + bias[item]
    return e_, q, out


def padded(R, inst, mask):
    """(ids [B, L], mask [B, L], items, n) of one side's instances"""
    I = R.shape[1]
    hist = [F.history(R, u, e) for u, _, e, _, _ in inst]
    L = max([len(x) for x in hist], default=0)
    ids = np.full((len(inst), L), I, np.int64)
    m = np.zeros((len(inst), L))
    for k, x in enumerate(hist):
        ids[k, :len(x)] = x
        m[k, :min(L, len(x) + (1 if mask == "reference" else 0))] = 1.0
    return ids, m, np.asarray([i for _, i, _, _, _ in inst], np.int64), np.asarray([float(x[3]) for x in inst]), hist


def step(st, R, users, items, third, pairwise, loss, regs, algorithm=0, activation=-1, alpha=0.0, beta=0.5,
         mask="reference", c1_rows=False):
    """one sess.run((loss, optimizer)): returns the pre-update loss (in st's width)"""
    dt = torch.float64 if st.var["c1"].dtype == np.float64 else torch.float32
    T = [torch.tensor(st.var[k], dtype=dt, requires_grad=True) for k in NAMES]
    inst = F.instances(R, users, items, third, pairwise)
    sides = [inst] if not pairwise else [inst[:len(inst) // 2], inst[len(inst) // 2:]]
    outs, e_s, q_s, hists, its = [], [], [], [], []
    for s in sides:
        ids, m, it, n, hist = padded(R, s, mask)
        e_, q, out = _side(T, torch.from_numpy(ids), torch.tensor(m, dtype=dt), torch.from_numpy(it),
                           torch.tensor(n, dtype=dt), algorithm, activation, alpha, beta)
        outs.append(out), e_s.append(e_), q_s.append(q), hists.extend(hist), its.append(it)
    if not pairwise:
        y = torch.tensor(np.asarray(third, np.float64), dtype=dt)
        x = outs[0]
        if loss == "square":
            total = ((y - x) ** 2).sum()
        else:
            total = (torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-torch.abs(x)))).mean()
        total = total + regs[0] * 0.5 * (e_s[0] ** 2).sum() + regs[1] * 0.5 * (q_s[0] ** 2).sum()
    else:
        yy = outs[0] - outs[1]
        if loss == "bpr":
            total = torch.nn.functional.softplus(-yy).sum()
        elif loss == "hinge":
            total = torch.clamp(yy + 1, min=0).sum()
        else:
            total = ((1 - yy) ** 2).sum()
        total = total + regs[0] * 0.5 * (e_s[0] ** 2).sum() + regs[1] * 0.5 * ((q_s[1] ** 2).sum() + (q_s[0] ** 2).sum())
    grads = torch.autograd.grad(total, T, allow_unused=True)
    G = {k: (np.zeros_like(st.var[k]) if g is None else g.numpy().astype(st.var[k].dtype)) for k, g in zip(NAMES, grads)}
    rows = np.unique(np.concatenate(its)) if its and len(np.concatenate(its)) else np.zeros(0, np.int64)
    hrows = np.unique(np.concatenate(hists)).astype(np.int64) if (c1_rows and hists) else None
    st.apply("c1", G["c1"], hrows)
    st.apply("Q", G["Q"], rows)
    st.apply("bias", G["bias"], rows)
    for k in ("W", "b", "h"):
        st.apply(k, G[k], None)
    st.b1p, st.b2p = st.b1p * 0.9, st.b2p * 0.999
    return float(total.detach())


def predict(R, T, users, algorithm=0, activation=-1, alpha=0.0, beta=0.5, dtype=torch.float64):
    """NAIS.py:246-257: the whole train row, the exact mask, n = |R_u|, every item; a user without train items scores
    the bias"""
    T = [torch.tensor(np.asarray(t, np.float64), dtype=dtype) for t in T]
    I = R.shape[1]
    out = np.empty((len(users), I))
    for k, u in enumerate(users):
        row = R.indices[R.indptr[u]:R.indptr[u + 1]].astype(np.int64)
        if not len(row):
            out[k] = T[2].numpy()
            continue
        ids = torch.from_numpy(np.tile(row, (I, 1)))
        _, _, o = _side(T, ids, torch.ones(ids.shape, dtype=dtype), torch.arange(I),
                        torch.full((I,), float(len(row)), dtype=dtype), algorithm, activation, alpha, beta)
        out[k] = o.numpy()
    return out
