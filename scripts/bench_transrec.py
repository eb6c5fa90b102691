"""Step time and scoring rate of the TransRec engine (neurec_amd/transrec.py) on the gowalla shape.

    python scripts/bench_transrec.py [--shape gowalla] [--steps 300] [--warmup 30] [--batch 1024] [--score-users 2048]

The train matrix is the synthetic gowalla-shaped one (neurec_amd/synth.py: the real degree distribution); every user's
time order is a seeded permutation of the row.  The instances come from the device stream of the time-order pairwise
sampler at high_order = 1, bpr / adam, reg_mf = 0 (conf/TransRec.properties).  Reported:

    step        d = 50, B = `--batch` (the shipped configuration): ms_per_step and instances_per_s over `--steps` engine
                steps timed between device events, after `--warmup` steps; grad_ms / apply_ms: the same batches through
                nrhip_transrec_step alone and through the four applications alone (launch-bound loops, not a split)
    score       at d = 50 and d = 64: engine.score() of `--score-users` test users against every item (median of 5,
                after one untimed call): ms, pairs/s, and the fraction of the VALU bound it reaches.  The direct form
                costs 2 n I d vector instructions (a subtract and a multiply-accumulate per pair and column); the bound
                is that count over the unpacked fp32 issue rate, VALU_RATE lane-instructions per second (a quarter of
                the 157.3 TFLOP/s vector peak, which counts a packed multiply-add as four)

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

VALU_RATE = 157.3e12 / 4


def _engine(train, d, batch):
    import numpy as np
    from neurec_amd.transrec import TransRecEngine
    U, I = train.shape
    rng = np.random.RandomState(2017)
    tabs = [(0.01 * rng.randn(*s)).astype(np.float32) for s in ((U, d), (I, d), (I,), (d,))]
    return TransRecEngine(*tabs, 0.001, 0.0, batch, loss="bpr", pairwise=True, learner="adam")


def bench_step(a, train, ds, d):
    import torch
    from neurec_amd.data import TimeOrderPairwiseSampler
    eng = _engine(train, d, a.batch)
    sampler = TimeOrderPairwiseSampler(ds, high_order=1, neg_num=1, batch_size=a.batch, shuffle=True, as_tensors=True)
    need = a.warmup + a.steps
    batches = []
    while len(batches) < need:
        for u, rec, it, neg in sampler:
            if u.numel() == a.batch:
                batches.append((u.clone(), rec.reshape(-1).clone(), it.clone(), neg.clone()))
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
    return {"d": d, "loss": "bpr", "learner": "adam", "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms, 4), "instances_per_s": round(a.batch / (ms * 1e-3), 1),
            "grad_ms": round(grad_ms, 4), "apply_ms": round(apply_ms, 4), "steps_per_epoch": len(sampler)}


def bench_score(a, train, test, ds, d):
    import numpy as np
    import torch
    eng = _engine(train, d, 1)
    U, I = train.shape
    last = np.full(U, -1, np.int32)
    for u, s in ds.seqs.items():
        last[u] = s[-1]
    last = torch.from_numpy(last).cuda()
    users = torch.from_numpy(np.flatnonzero(np.diff(test.indptr) > 0).astype(np.int32)[:a.score_users]).cuda()
    times = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(6):
        torch.cuda.synchronize()
        e0.record()
        S = eng.score(users, last)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    assert bool(torch.isfinite(S).all())
    ms = sorted(times[1:])[2]
    n = int(users.numel())
    bound_ms = 2.0 * n * I * d / VALU_RATE * 1e3
    return {"d": d, "score_users": n, "items": I, "score_ms": round(ms, 3),
            "score_pairs_per_s": round(n * I / (ms * 1e-3), 1), "valu_instructions": 2 * n * I * d,
            "valu_bound_ms": round(bound_ms, 4), "fraction_of_valu_bound": round(bound_ms / ms, 3)}


def bench(a):
    from neurec_amd import synth
    train, test = synth.interactions(a.shape)
    train, test = train.tocsr(), test.tocsr()
    train.sort_indices()
    ds = _Dataset(train)
    return {"script": "scripts/bench_transrec.py", "shape": a.shape, "users": train.shape[0], "items": train.shape[1],
            "nnz": int(train.nnz), "step": bench_step(a, train, ds, 50),
            "score": [bench_score(a, train, test, ds, d) for d in (50, 64)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="gowalla")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--score-users", type=int, default=2048)
    print(json.dumps(bench(ap.parse_args())), flush=True)


if __name__ == "__main__":
    main()
