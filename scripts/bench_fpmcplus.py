"""Step time and scoring rate of the FPMCplus engine (neurec_amd/fpmcplus.py) on the gowalla shape.

    python scripts/bench_fpmcplus.py [--shape gowalla] [--steps 300] [--warmup 30] [--order 3] [--weight 16]
                                     [--score-users 2048]

The train matrix is the synthetic gowalla-shaped one (neurec_amd/synth.py: the real degree distribution); every user's
time order is a seeded permutation of the row.  The instances come from the device stream of the time-order pairwise
sampler at high_order = `--order` (conf/FPMCplus.properties: 3), bpr / adam, reg_mf = 1e-5, reg_w = 1e-3,
weight_size = `--weight` (16).  Four configurations: d = 16 (the reference's) and d = 64, each at B = 128 (the
reference's) and B = 256.  Reported per configuration:

    ms_per_step, instances_per_s   `--steps` engine steps timed between device events, after `--warmup` steps
    grad_ms, apply_ms              the same batches through nrhip_fpmcplus_step alone and through the seven
                                   applications alone (the gradient buffers are zero then: the sweep's traffic is the same)
    score_ms, score_pairs_per_s, score_tanh_per_s
                                   engine.score() of `--score-users` test users against every item (median of 5, after
                                   one untimed call): n I pairs, n I L w tanh

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


def bench_one(a, train, test, ds, d, batch):
    import numpy as np
    import torch
    from neurec_amd.data import TimeOrderPairwiseSampler
    from neurec_amd.fpmcplus import FPMCplusEngine, last_items_table
    U, I = train.shape
    L, w = a.order, a.weight
    rng = np.random.RandomState(2017)
    tabs = [(0.01 * rng.randn(n, d)).astype(np.float32) for n in (U, I, I, I)]
    tabs += [(rng.randn(3 * d, w) * np.sqrt(2.0 / (3 * d))).astype(np.float32),
             (rng.randn(w) * np.sqrt(2.0)).astype(np.float32), np.ones(w, np.float32)]
    reg_mf, reg_w, lr = 1e-5, 1e-3, 0.001                      # conf/FPMCplus.properties
    eng = FPMCplusEngine(*tabs, lr, reg_mf, reg_w, batch, L, loss="bpr", pairwise=True, learner="adam",
                         last_items=last_items_table(ds.seqs, U, L))
    sampler = TimeOrderPairwiseSampler(ds, high_order=L, batch_size=batch, shuffle=True, as_tensors=True)
    need = a.warmup + a.steps
    batches = []
    while len(batches) < need:
        for u, rec, it, neg in sampler:
            if u.numel() == batch:
                batches.append((u.clone(), rec.reshape(-1, L).clone(), it.clone(), neg.clone()))
            if len(batches) == need:
                break
    losses = torch.zeros((need, 2), device="cuda")
    for k in range(a.warmup):
        eng.step(*batches[k], losses[k])
    ms = _timed(lambda k: eng.step(*batches[a.warmup + k], losses[a.warmup + k]), a.steps)
    assert bool(torch.isfinite(losses).all())
    grad_ms = _timed(lambda k: eng.gradients(*batches[a.warmup + k], losses[a.warmup + k]), a.steps)
    for g in eng.G.values():
        g.zero_()
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    users = np.flatnonzero(np.diff(test.indptr) > 0).astype(np.int32)[:a.score_users]
    users = torch.from_numpy(users).cuda()
    times = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(6):
        torch.cuda.synchronize()
        e0.record()
        S = eng.score(users)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    assert bool(torch.isfinite(S).all())
    score_ms = sorted(times[1:])[2]
    n = int(users.numel())
    return {"d": d, "w": w, "high_order": L, "loss": "bpr", "learner": "adam", "batch": batch, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(ms, 4), "instances_per_s": round(batch / (ms * 1e-3), 1),
            "grad_ms": round(grad_ms, 4), "apply_ms": round(apply_ms, 4), "steps_per_epoch": len(sampler),
            "score_users": n, "score_ms": round(score_ms, 3),
            "score_users_per_s": round(n / (score_ms * 1e-3), 1),
            "score_pairs_per_s": round(n * I / (score_ms * 1e-3), 1),
            "score_tanh_per_s": round(n * I * L * w / (score_ms * 1e-3), 1)}


def bench(a):
    from neurec_amd import synth
    train, test = synth.interactions(a.shape)
    train, test = train.tocsr(), test.tocsr()
    train.sort_indices()
    ds = _Dataset(train)
    runs = [bench_one(a, train, test, ds, d, batch) for d in (16, 64) for batch in (128, 256)]
    return {"script": "scripts/bench_fpmcplus.py", "shape": a.shape, "users": train.shape[0], "items": train.shape[1],
            "nnz": int(train.nnz), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="gowalla")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--weight", type=int, default=16)
    ap.add_argument("--score-users", type=int, default=2048)
    print(json.dumps(bench(ap.parse_args())), flush=True)


if __name__ == "__main__":
    main()
