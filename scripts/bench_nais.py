"""Step time and scoring rate of the NAIS engine (neurec_amd/nais.py) on the gowalla shape, shipped config.

    python scripts/bench_nais.py [--shape gowalla] [--steps 500] [--warmup 50] [--batch 256] [--d 16] [--w 16]
                                 [--score-block 1024] [--score-blocks 0] [--fism-steps 500]
                                 [--torch-steps 30] [--eval 1] [--c1-path walk|sort] [--pair-kernel auto|valu|mfma]

The train matrix is the synthetic gowalla-shaped one (neurec_amd/synth.py); the instances come from the device stream
(PointwiseSampler, num_neg = 4), algorithm 0, no activation, cross-entropy, adam, alpha = 0, beta = 0.5:
conf/NAIS.properties as shipped.  Reported:

    ms_per_step, instances_per_s   `--steps` engine steps timed between device events, after `--warmup` steps
    score_ms_per_block, score_users_per_s
                                   score() of blocks of `--score-block` users ([B, I] each; `--score-blocks` of them,
                                   0 = every user), and the share of the fp32 FMA peak the pair kernel's
                                   I |H*| d w multiply-adds reach in that time (the whole call is charged to them)
    eval_ms, eval_users_per_s      the evaluation of every test user in blocks of `--score-block`: score(), the train
                                   items masked, top-20 and the five metrics (engine.mask_train / eval_scores)
    fism_ms_per_step               for scale: FISMEngine.step on the same batches (square loss)
    torch_ms_per_step              for scale: the reference's formulation restated in plain torch on the device — the
                                   batch padded to [B, Lmax] on the host beforehand (not timed), `c1` with a zero pad
                                   row gathered to [B, Lmax, d], the attention MLP on it, the reference's mask,
                                   autograd, torch.optim.Adam on the six tables — over `--torch-steps` of the batches

One JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.bench_fism import _Dataset       # noqa: E402

FP32_FMA_PEAK = 78.6e12                       # MI355X vector fp32, FLOP/s without packed math (2 per FMA)


def _torch_steps(train, T, batches, beta, regs, lr):
    """ms per step of the padded-gather + autograd restatement over `batches` (host tuples)"""
    import numpy as np
    import torch
    c1, Q, W, b = T
    I, d = c1.shape
    dev = "cuda"
    P = [torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(x)).to(dev)) for x in (c1, Q, W, b)]
    bias = torch.nn.Parameter(torch.zeros(I, device=dev))
    h = torch.nn.Parameter(torch.ones(W.shape[1], device=dev))
    opt = torch.optim.Adam(P + [bias, h], lr=lr)
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
    pad = torch.zeros((1, d), device=dev)

    def one(H, n, items, labels):
        e_ = torch.cat([P[0], pad], 0)[H]
        q = P[1][items]
        ex = torch.exp(((e_ * q[:, None, :]) @ P[2] + P[3]) @ h)
        ex = ex * (torch.arange(H.shape[1], device=dev)[None, :] < n[:, None])
        p = ((ex / ex.sum(1, keepdim=True).pow(beta))[:, :, None] * e_).sum(1)
        out = (p * q).sum(1) + bias[items]
        loss = torch.nn.functional.binary_cross_entropy_with_logits(out, labels) \
            + regs[0] * 0.5 * (e_ * e_).sum() + regs[1] * 0.5 * (q * q).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    for f in feeds[:3]:
        one(*f)
    return _timed(lambda k: one(*feeds[k]), len(feeds))


def _timed(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for k in range(n):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / max(n, 1)


def bench(a):
    import numpy as np
    import torch
    from neurec_amd import synth
    from neurec_amd.data import PointwiseSampler
    from neurec_amd.fism import FISMEngine
    from neurec_amd.nais import NAISEngine
    train, test = synth.interactions(a.shape)
    train = train.tocsr()
    train.sort_indices()
    U, I = train.shape
    rng = np.random.RandomState(2017)
    c1 = (0.01 * rng.randn(I, a.d)).astype(np.float32)
    Q = (0.01 * rng.randn(I, a.d)).astype(np.float32)
    W = (rng.randn(a.d, a.w) * np.sqrt(2.0 / a.d)).astype(np.float32)
    b = (0.01 * rng.randn(a.w)).astype(np.float32)
    eng = NAISEngine(c1, Q, W, b, train, 0.001, [1e-7, 1e-7, 1e-5], 0.0, 0.5, a.batch, algorithm=0, activation="Relu",
                     loss="cross_entropy", learner="adam", c1_path=a.c1_path, pair_kernel=a.pair_kernel)
    sampler = PointwiseSampler(_Dataset(train), neg_num=4, batch_size=a.batch, shuffle=True, as_tensors=True)
    need = a.warmup + max(a.steps, a.fism_steps)
    batches = []
    while len(batches) < need:
        for bt in sampler:
            if bt[0].numel() == a.batch:
                batches.append(bt)
            if len(batches) == need:
                break
    losses = torch.zeros((need, 2), device="cuda")
    most = eng.max_positions([bt[0] for bt in batches])       # as the plugin, once per epoch
    for k in range(a.warmup):
        eng.step(*batches[k], losses[k], positions=most)
    ms = _timed(lambda k: eng.step(*batches[a.warmup + k], losses[a.warmup + k], positions=most), a.steps)
    eng.verify()
    assert bool(torch.isfinite(losses).all())
    out = {"c1_path": a.c1_path, "pair_kernel": "mfma" if eng.mfma else "valu", "shape": a.shape, "users": U, "items": I, "nnz": int(train.nnz), "d": a.d, "w": a.w, "batch": a.batch,
           "num_neg": 4, "loss": "cross_entropy", "learner": "adam", "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": round(ms, 4), "instances_per_s": round(a.batch / (ms * 1e-3), 1),
           "row_buffer_mb": round(eng._rows.numel() * 4 / 2**20, 1)}
    if a.fism_steps:
        fism = FISMEngine(c1, Q, train, 0.001, [1e-7, 1e-7], 0.5, a.batch, loss="square", learner="adam")
        for k in range(a.warmup):
            fism.step(*batches[k], losses[k])
        out["fism_ms_per_step"] = round(_timed(lambda k: fism.step(*batches[a.warmup + k], losses[a.warmup + k]),
                                               a.fism_steps), 4)
    if a.torch_steps:
        host = [tuple(t.cpu().numpy() for t in bt) for bt in batches[a.warmup:a.warmup + a.torch_steps]]
        out["torch_ms_per_step"] = round(_torch_steps(train, (c1, Q, W, b), host, 0.5, [1e-7, 1e-7], 0.001), 3)
        out["torch_steps"] = a.torch_steps
    if a.eval:
        from neurec_amd import engine as E
        test = test.tocsr()
        tr, te = E.DeviceCSR.from_scipy(train), E.DeviceCSR.from_scipy(test)
        tu = np.flatnonzero(np.diff(test.indptr) > 0).astype(np.int32)
        tblocks = [tu[s:s + a.score_block] for s in range(0, len(tu), a.score_block)]

        def ev(k):
            S = eng.score(tblocks[k])
            du = torch.from_numpy(tblocks[k]).cuda()
            E.mask_train(S, du, tr)
            E.eval_scores(S, te, [1, 2, 3, 4, 5], 20, users=du)
        ev(0)
        ems = _timed(ev, len(tblocks)) * len(tblocks)
        out.update({"eval_users": int(len(tu)), "eval_ms": round(ems, 1),
                    "eval_users_per_s": round(len(tu) / (ems * 1e-3), 1)})
    blocks = [np.arange(s, min(s + a.score_block, U), dtype=np.int32) for s in range(0, U, a.score_block)]
    if a.score_blocks:
        blocks = blocks[:a.score_blocks]
    eng.score(blocks[0])
    sms = _timed(lambda k: eng.score(blocks[k]), len(blocks))
    hstar = float(np.mean([len(np.unique(train[bl].indices)) for bl in blocks]))
    flops = 2.0 * I * hstar * a.d * a.w
    out.update({"score_block": a.score_block, "score_blocks": len(blocks), "score_ms_per_block": round(sms, 3),
                "score_users_per_s": round(sum(len(bl) for bl in blocks) / (sms * len(blocks) * 1e-3), 1),
                "score_measured_users": int(sum(len(bl) for bl in blocks)),
                "distinct_history_items_per_block": round(hstar, 1),
                "pair_fma_share_of_fp32_peak": round(flops / (sms * 1e-3) / FP32_FMA_PEAK, 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="gowalla")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--w", type=int, default=16)
    ap.add_argument("--score-block", type=int, default=1024)
    ap.add_argument("--score-blocks", type=int, default=0)
    ap.add_argument("--fism-steps", type=int, default=500)
    ap.add_argument("--torch-steps", type=int, default=30)
    ap.add_argument("--eval", type=int, default=1)
    ap.add_argument("--c1-path", default="walk", choices=["walk", "sort"])
    ap.add_argument("--pair-kernel", default="auto", choices=["auto", "valu", "mfma"])
    print(json.dumps(bench(ap.parse_args())), flush=True)


if __name__ == "__main__":
    main()
