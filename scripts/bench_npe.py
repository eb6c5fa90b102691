"""Step time and evaluation rate of the NPE engine (neurec_amd/npe.py) on the gowalla shape.

    python scripts/bench_npe.py [--shape gowalla] [--steps 300] [--warmup 30] [--batch 256] [--order 3]
                                [--torch-steps 100]

The train matrix is the synthetic gowalla-shaped one (neurec_amd/synth.py: the real degree distribution); every user's
time order is a seeded permutation of the row.  The instances come from the device stream of the time-order pointwise
sampler at high_order = `--order` (conf/NPE.properties: 3), num_neg = 4, cross_entropy / adam, reg = 0.1.  Two
configurations: the reference's d = 64 and d = 16.  Reported per configuration:

    ms_per_step, instances_per_s   `--steps` engine steps timed between device events, after `--warmup` steps
    grad_ms, apply_ms              the same batches through nrhip_npe_step alone and through the three applications
                                   alone (the gradient buffers are zero then: the sweep's traffic is the same)
    eval_users_per_s               user factors h_u and relu(V) at width d + the full-rank evaluation of every test user
                                   on the factor path (median of 5)
    torch_ms_per_step              the same step in torch eager ops on the same GPU: index_select gathers, relu, the
                                   gates as indicators, index_add_ into dense gradient buffers, the same sweeping Adam
                                   on the three tables — over `--torch-steps` of the same batches; for context only

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

from bench_fpmc import _Dataset, _timed          # noqa: E402


def _torch_steps(tabs, batches, L, reg, lr):
    """ms per step of the eager restatement over `batches` (device tuples)"""
    import torch
    T = [torch.from_numpy(t).to("cuda") for t in tabs]
    G = [torch.zeros_like(t) for t in T]
    M = [torch.zeros_like(t) for t in T]
    V2 = [torch.zeros_like(t) for t in T]
    Pt, Vt, Wt = T
    d = Pt.shape[1]
    state = {"b1p": 0.9, "b2p": 0.999}

    def one(k):
        u, rec, i, y = batches[k % len(batches)]
        p, v = Pt.index_select(0, u), Vt.index_select(0, i)
        rows = Wt.index_select(0, rec.reshape(-1)).view(-1, L, d)
        s = rows.sum(1)
        q, rv = torch.relu(p) + torch.relu(s), torch.relu(v)
        x = (rv * q).sum(1)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(x, y) + \
            reg * 0.5 * ((p * p).sum() + (rows * rows).sum() + (v * v).sum())
        g = ((torch.sigmoid(x) - y) / x.numel())[:, None]
        grv = g * rv
        G[0].index_add_(0, u, grv * (p > 0) + reg * p)
        G[1].index_add_(0, i, g * q * (v > 0) + reg * v)
        G[2].index_add_(0, rec.reshape(-1), ((grv * (s > 0))[:, None, :] + reg * rows).reshape(-1, d))
        alpha = lr * (1 - state["b2p"]) ** 0.5 / (1 - state["b1p"])
        for t, gr, m, v2 in zip(T, G, M, V2):                  # TF-1.12's sparse Adam: every row swept
            m.mul_(0.9).add_(gr, alpha=0.1)
            v2.mul_(0.999).addcmul_(gr, gr, value=0.001)
            t.addcdiv_(m, v2.sqrt().add_(1e-8), value=-alpha)
            gr.zero_()
        state["b1p"] *= 0.9
        state["b2p"] *= 0.999
        return loss
    for k in range(5):
        one(k)
    return _timed(one, len(batches))


def bench_one(a, train, test, ds, d):
    import numpy as np
    import torch
    from neurec_amd import engine as E
    from neurec_amd.data import TimeOrderPointwiseSampler
    from neurec_amd.model.sequential_recommender.HRM import last_items_table
    from neurec_amd.npe import NPEEngine
    from neurec_amd.trainer import FullRankEvaluator
    U, I = train.shape
    L = a.order
    rng = np.random.RandomState(2017)
    tabs = [(0.01 * rng.randn(n, d)).astype(np.float32) for n in (U, I, I)]
    reg, lr = 0.1, 0.001                                       # conf/NPE.properties
    eng = NPEEngine(*tabs, lr, reg, a.batch, L, loss="cross_entropy", learner="adam",
                    last_items=last_items_table(ds.seqs, U, L))
    sampler = TimeOrderPointwiseSampler(ds, high_order=L, neg_num=4, batch_size=a.batch, shuffle=True, as_tensors=True)
    need = a.warmup + a.steps
    batches = []
    while len(batches) < need:
        for u, rec, it, y in sampler:
            if u.numel() == a.batch:
                batches.append((u.clone(), rec.reshape(-1, L).clone(), it.clone(), y.clone()))
            if len(batches) == need:
                break
    losses = torch.zeros((need, 2), device="cuda")
    for k in range(a.warmup):
        eng.step(*batches[k], losses[k])
    ms = _timed(lambda k: eng.step(*batches[a.warmup + k], losses[a.warmup + k]), a.steps)
    assert bool(torch.isfinite(losses).all())
    # the split: the C call alone (its rows of G are overwritten by the next call, never applied), then the three
    # applications alone on zero gradients
    grad_ms = _timed(lambda k: eng.gradients(*batches[a.warmup + k], losses[a.warmup + k]), a.steps)
    for g in eng.G.values():
        g.zero_()
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    ranker = FullRankEvaluator(E.DeviceCSR.from_scipy(train), E.DeviceCSR.from_scipy(test), [1, 2, 3, 4, 5], 20)
    users = torch.from_numpy(np.flatnonzero(np.diff(test.indptr) > 0).astype(np.int32)).cuda()
    times = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(6):
        torch.cuda.synchronize()
        e0.record()
        result = ranker.evaluate_factors(eng.user_factors(), eng.item_factors(), users, exact_mean=True)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    eval_ms = sorted(times[1:])[2]
    torch_ms = None
    if a.torch_steps:
        dev_batches = [tuple(t.long() if t.dtype == torch.int32 else t for t in bt)
                       for bt in batches[a.warmup:a.warmup + a.torch_steps]]
        torch_ms = _torch_steps(tabs, dev_batches, L, reg, lr)
    return {"d": d, "loss": "cross_entropy", "learner": "adam", "high_order": L, "reg": reg, "num_neg": 4,
            "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 4),
            "instances_per_s": round(a.batch / (ms * 1e-3), 1), "grad_ms": round(grad_ms, 4),
            "apply_ms": round(apply_ms, 4), "steps_per_epoch": len(sampler), "eval_width": d,
            "eval_users": int(users.numel()), "eval_ms": round(eval_ms, 3),
            "eval_users_per_s": round(users.numel() / (eval_ms * 1e-3), 1),
            "ndcg_at_10": float(np.asarray(result)[3 * 20 + 9]),
            "torch_ms_per_step": None if torch_ms is None else round(torch_ms, 4), "torch_steps": a.torch_steps,
            "torch_over_engine": None if torch_ms is None else round(torch_ms / ms, 2)}


def bench(a):
    from neurec_amd import synth
    train, test = synth.interactions(a.shape)
    train, test = train.tocsr(), test.tocsr()
    train.sort_indices()
    ds = _Dataset(train)
    runs = [bench_one(a, train, test, ds, d) for d in (64, 16)]
    return {"shape": a.shape, "users": train.shape[0], "items": train.shape[1], "nnz": int(train.nnz), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="gowalla")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=100)
    print(json.dumps(bench(ap.parse_args())), flush=True)


if __name__ == "__main__":
    main()
