"""Step time and score() throughput of the DeepICF engine (neurec_amd/deepicf.py) at the reference's defaults on the
gowalla shape, beside NAIS's own step (the floor: DeepICF does strictly more) and torch-on-device statements of the
same step and of the same scores.

    python scripts/bench_deepicf.py [--steps 200] [--warmup 30] [--repeats 5] [--batch 256] [--torch-steps 20]
                                    [--score-users 1024] [--torch-score-users 16] [--pair-kernel auto|valu|mfma]

conf/DeepICF.properties: embedding_size 16, weight_size 16, layers [64,32,16], algorithm 1, no activation, batch norm,
batch 256, adam, lr 0.001, regs [1e-6, 1e-6, 1e-5], regw [10, 10].  The train matrix is the synthetic gowalla-shaped
one (neurec_amd/synth.py: U = 29,858, I = 40,981); the instances come from the device stream (PointwiseSampler,
num_neg = 4).  In ONE process, `--repeats` windows of `--steps` steps of the engine, of NAIS's engine on the same
batches (same d, w, algorithm, batch) and of `--torch-steps` steps of the torch statement, INTERLEAVED, each timed
between device events after a warm-up: the median window and the range, in ms per step.

    engine          ms_per_step (median, min, max), grad_ms / apply_ms (nrhip_deepicf_step alone, the learner's
                    applications alone), launches per step
    nais            the same batches through NAISEngine.step; engine_over_nais is the ratio
    torch           the step as torch ops on the device: the batch padded to [B, Lmax] on the host beforehand (not
                    timed), `c1` with a zero pad row gathered to [B, Lmax, d], the attention MLP on the concatenation,
                    the reference's mask, the tower with torch's batch norm, the log loss, the whole-table
                    regularisers, autograd, torch.optim.Adam on every variable
    score           users / s of score() and TFLOP/s on the per-pair count (2 |R_u| d of the pooling at the mean row
                    length, 2 sum in_k out_k of the tower, 2 layers[-1] of the output) against the 155 TF fp32-MFMA
                    ceiling; full_eval_ms: all U users at that rate
    torch_score     the same scores with torch ops, a user at a time ([I, |R_u|, w] materialised)

One JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_fpmc import _timed          # noqa: E402
from scripts.bench_fism import _Dataset       # noqa: E402

MFMA_F32_RATE = 155e12
D, W, LAYERS, LR = 16, 16, [64, 32, 16], 0.001
REGS, REGW, BETA = [1e-6, 1e-6, 1e-5], [10.0, 10.0], 0.5
BN_EPS = 0.001


def _tables(I, seed=2017):
    import numpy as np
    rs = np.random.RandomState(seed)
    f = lambda x: x.astype(np.float32)
    T = dict(c1=f(0.01 * rs.randn(I, D)), Q=f(0.01 * rs.randn(I, D)), W=f(rs.randn(2 * D, W) * np.sqrt(1.0 / D)),
             b=f(0.01 * rs.randn(W)), Wout=f(rs.randn(LAYERS[-1], 1) * np.sqrt(2.0 / LAYERS[-1])), bout=f(rs.randn(1)))
    n_in = D
    for k, n in enumerate(LAYERS):
        T["W%d" % k], T["b%d" % k] = f(rs.randn(n_in, n) * np.sqrt(2.0 / n_in)), f(rs.randn(n))
        n_in = n
    return T


def _torch_step_fn(train, T, batches):
    """the padded feeds of `batches` (host tuples) and fn(k): the step as torch ops + autograd + torch.optim.Adam"""
    import numpy as np
    import torch
    dev = "cuda"
    I = train.shape[1]
    P = {k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(v)).to(dev)) for k, v in T.items()}
    P["bias"] = torch.nn.Parameter(torch.zeros(I, device=dev))
    P["h"] = torch.nn.Parameter(torch.ones(W, device=dev))
    bn = [torch.nn.BatchNorm1d(n, eps=BN_EPS, momentum=0.1).to(dev) for n in LAYERS]
    opt = torch.optim.Adam(list(P.values()) + [p for m in bn for p in m.parameters()], lr=LR)
    deg = np.diff(train.indptr)
    feeds = []
    for users, items, labels in batches:
        L = max(int(deg[users].max()), 1)
        H = np.full((len(users), L), I, np.int64)
        n = np.empty(len(users), np.float32)
        for k, (u, i, y) in enumerate(zip(users, items, labels)):
            row = train.indices[train.indptr[u]:train.indptr[u + 1]]
            if y > 0.5:
                row = row[row != i]
            H[k, :len(row)] = row
            n[k] = len(row) + 1
        feeds.append(tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev)
                           for x in (H, n, items.astype(np.int64), labels)))
    pad = torch.zeros((1, D), device=dev)

    def one(k):
        H, n, items, labels = feeds[k % len(feeds)]
        e_ = torch.cat([P["c1"], pad], 0)[H]
        q = P["Q"][items]
        x = torch.cat([e_, q[:, None, :].expand(-1, e_.shape[1], -1)], 2)
        ex = torch.exp((x @ P["W"] + P["b"]) @ P["h"])
        ex = ex * (torch.arange(H.shape[1], device=dev)[None, :] < n[:, None])
        p = ((ex / ex.sum(1, keepdim=True).pow(BETA))[:, :, None] * e_).sum(1)
        x = p * q
        for j in range(len(LAYERS)):
            x = torch.relu(bn[j](x @ P["W%d" % j] + P["b%d" % j]))
        prob = torch.sigmoid((x @ P["Wout"] + P["bout"]).sum(1) + P["bias"][items])
        loss = (-labels * torch.log(prob + 1e-7) - (1 - labels) * torch.log(1 - prob + 1e-7)).mean() \
            + REGS[0] * 0.5 * (P["Q"] ** 2).sum() + REGS[1] * 0.5 * (P["c1"] ** 2).sum() \
            + REGS[2] * 0.5 * (P["W"] ** 2).sum() + sum(r * 0.5 * (P["W%d" % j] ** 2).sum() for j, r in enumerate(REGW))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return one


def _torch_score_fn(train, eng):
    """[n, I] scores with torch ops, a user at a time, from the engine's tables as the steps left them"""
    import torch
    g = lambda k: getattr(eng, k)
    I = train.shape[1]
    indptr, indices = train.indptr, train.indices

    def score(users):
        out = torch.empty((len(users), I), device="cuda")
        with torch.no_grad():
            cW, qW = g("c1") @ g("W")[:D], g("Q") @ g("W")[D:] + g("b")
            for r, u in enumerate(users):
                row = torch.from_numpy(indices[indptr[u]:indptr[u + 1]].astype("int64")).to("cuda")
                e = torch.exp((cW[row][None, :, :] + qW[:, None, :]) @ g("h"))              # [I, L]
                x = ((e / e.sum(1, keepdim=True).pow(BETA)) @ g("c1")[row]) * g("Q")
                for j in range(len(LAYERS)):
                    z = x @ g("W%d" % j) + g("b%d" % j)
                    z = g("gamma%d" % j) * (z - eng.mm[j]) / torch.sqrt(eng.mv[j] + BN_EPS) + g("beta%d" % j)
                    x = torch.relu(z)
                out[r] = torch.sigmoid(x @ g("Wout") + g("bout") + g("bias"))
        return out
    return score


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--torch-steps", type=int, default=20)
    ap.add_argument("--score-users", type=int, default=1024)
    ap.add_argument("--torch-score-users", type=int, default=16)
    ap.add_argument("--pair-kernel", default="auto")
    a = ap.parse_args()
    from neurec_amd import synth
    from neurec_amd.data import PointwiseSampler
    from neurec_amd.deepicf import DeepICFEngine
    from neurec_amd.nais import NAISEngine
    train, _ = synth.interactions("gowalla")
    train = train.tocsr()
    train.sort_indices()
    U, I = train.shape
    T = _tables(I)
    tower = {k: v for k, v in T.items() if k not in ("c1", "Q", "W", "b")}
    eng = DeepICFEngine(T["c1"], T["Q"], T["W"], T["b"], tower, train, LR, REGS, REGW, 0.0, BETA, a.batch, algorithm=1,
                        activation="Relu", batch_norm=True, pair_kernel=a.pair_kernel)
    nais = NAISEngine(T["c1"], T["Q"], T["W"], T["b"], train, LR, [1e-7, 1e-7, 1e-5], 0.0, BETA, a.batch, algorithm=1,
                      activation="Relu", loss="cross_entropy", learner="adam")
    sampler = PointwiseSampler(_Dataset(train), neg_num=4, batch_size=a.batch, shuffle=True, as_tensors=True)
    n_feed, batches = 64, []
    for bt in sampler:
        if bt[0].numel() == a.batch:
            batches.append(bt)
        if len(batches) == n_feed:
            break
    positions = eng.max_positions([b[0] for b in batches])
    dev = eng.c1.device
    loss2 = torch.zeros(2, device=dev)
    step = lambda k: eng.step(*batches[k % n_feed], loss2, positions=positions)
    nstep = lambda k: nais.step(*batches[k % n_feed], loss2, positions=positions)
    _timed(step, a.warmup)
    _timed(nstep, a.warmup)
    tstep = None
    if a.torch_steps:
        host = [tuple(x.cpu().numpy() for x in b) for b in batches[:a.torch_steps]]
        tstep = _torch_step_fn(train, dict(T), host)
        _timed(tstep, 3)
    we, wn, wt = [], [], []
    for _ in range(a.repeats):                                   # interleaved: all see the same state of the machine
        we.append(_timed(step, a.steps))
        wn.append(_timed(nstep, a.steps))
        if tstep is not None:
            wt.append(_timed(tstep, a.torch_steps))
    eng.verify()
    for w in (we, wn, wt):
        w.sort()
    mid = lambda w: {"ms_per_step": w[len(w) // 2], "min": w[0], "max": w[-1]}
    grad_ms = _timed(lambda k: eng.gradients(*batches[k % n_feed], loss2), a.steps)
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    L = len(LAYERS)
    launches = {"nrhip_deepicf_step": 2 + 4 + 2 * L + 1 + 1 + 2 * L + 1 + 4 + 3, "apply": len(eng._names)}
    out = {"shape": {"n_users": U, "n_items": I, "nnz": int(train.nnz), "embedding_size": D, "weight_size": W,
                     "layers": LAYERS, "batch": a.batch, "positions": int(positions)},
           "engine": dict(mid(we), grad_ms=grad_ms, apply_ms=apply_ms, launches=launches,
                          launches_per_step=sum(launches.values())),
           "nais": mid(wn)}
    out["engine_over_nais"] = out["engine"]["ms_per_step"] / out["nais"]["ms_per_step"]
    if wt:
        out["torch"] = mid(wt)
        out["engine_over_torch"] = out["engine"]["ms_per_step"] / out["torch"]["ms_per_step"]

    # ---- score(): every item for n users
    rs = np.random.RandomState(1)
    su = rs.randint(0, U, a.score_users).astype(np.int32)
    mean_row = float(np.diff(train.indptr)[su].mean())
    ins = [D] + LAYERS[:-1]
    flop_per_pair = 2 * mean_row * D + 2 * sum(i * w for i, w in zip(ins, LAYERS)) + 2 * LAYERS[-1]
    score = lambda k: eng.score(su)
    _timed(score, 2)
    sm = sorted(_timed(score, 3) for _ in range(5))
    ms = sm[len(sm) // 2]
    n = a.score_users
    out["score"] = {"users": n, "tower": "mfma" if eng.tower_mfma else "valu", "ms": ms, "min": sm[0], "max": sm[-1],
                    "users_per_s": n / ms * 1e3, "mean_row": mean_row, "flop_per_pair": flop_per_pair,
                    "tflops": n * I * flop_per_pair / ms / 1e9,
                    "of_ceiling": n * I * flop_per_pair / ms / 1e9 / (MFMA_F32_RATE / 1e12),
                    "full_eval_ms": U / (n / ms)}
    if a.torch_score_users:
        nt = a.torch_score_users
        tscore_fn = _torch_score_fn(train, eng)
        tscore = lambda k: tscore_fn(su[:nt])
        _timed(tscore, 1)
        tm = sorted(_timed(tscore, 2) for _ in range(3))[1]
        out["torch_score"] = {"users": nt, "ms": tm, "users_per_s": nt / tm * 1e3, "full_eval_ms": U / (nt / tm)}
        out["score_over_torch"] = out["score"]["users_per_s"] / out["torch_score"]["users_per_s"]
        got, want = eng.score(su[:nt]), tscore_fn(su[:nt])
        out["score_vs_torch"] = {"max_err": float((got - want).abs().max()), "max_abs": float(want.abs().max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
