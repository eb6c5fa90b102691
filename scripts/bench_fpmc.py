"""Step time and evaluation rate of the FPMC engine (neurec_amd/fpmc.py) on the gowalla shape.

    python scripts/bench_fpmc.py [--shape gowalla] [--steps 500] [--warmup 50] [--batch 512] [--torch-steps 100]

The train matrix is the synthetic gowalla-shaped one (neurec_amd/synth.py: the real degree distribution); every user's
time order is a seeded permutation of the row.  The instances come from the device streams of the time-order samplers
at high_order = 1.  Four configurations: pairwise bpr / adam and pointwise cross_entropy / adam (num_neg = 4), each at
d = 64 and at the reference's default d = 16.  Reported per configuration:

    ms_per_step, instances_per_s   `--steps` engine steps timed between device events, after `--warmup` steps
    grad_ms, apply_ms              the same batches through nrhip_fpmc_step alone and through the four applications
                                   alone (the gradient buffers are zero then: the sweep's traffic is the same)
    sweep_gbytes_per_s             the applications' algorithmic bytes (per table element: var, m, v, grad read, var, m,
                                   v written and grad cleared: 32 B) over apply_ms
    eval_users_per_s               user and item factors at width 2 d + the full-rank evaluation of every test user on
                                   the factor path (median of 5)
    torch_ms_per_step              the same step in torch eager ops on the same GPU: index_select, index_add_ into dense
                                   gradient buffers, the same sweeping Adam on the four tables — over `--torch-steps` of
                                   the same batches

One JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class _Dataset:
    """what the time-order samplers ask of data.dataset.Dataset"""

    def __init__(self, train, seed=7):
        import numpy as np
        self.train_matrix = train
        self.num_users, self.num_items = train.shape
        rs = np.random.RandomState(seed)
        self.seqs = {u: rs.permutation(train.indices[train.indptr[u]:train.indptr[u + 1]]).tolist()
                     for u in range(train.shape[0]) if train.indptr[u + 1] > train.indptr[u]}

    def get_user_train_dict(self, by_time=False):
        return {u: (list(s) if by_time else sorted(s)) for u, s in self.seqs.items()}


def _timed(fn, n):
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(n):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _torch_steps(tabs, batches, pairwise, reg, lr):
    """ms per step of the eager restatement over `batches` (device tuples)"""
    import torch
    dev = "cuda"
    T = [torch.from_numpy(t).to(dev) for t in tabs]
    G = [torch.zeros_like(t) for t in T]
    M = [torch.zeros_like(t) for t in T]
    V = [torch.zeros_like(t) for t in T]
    UI, IU, IL, LI = T
    state = {"b1p": 0.9, "b2p": 0.999}

    def one(k):
        u, l, i, third = batches[k % len(batches)]
        ui, li, iu, il = UI.index_select(0, u), LI.index_select(0, l), IU.index_select(0, i), IL.index_select(0, i)
        x = (ui * iu).sum(1) + (il * li).sum(1)
        if pairwise:
            ju, jl = IU.index_select(0, third), IL.index_select(0, third)
            y = x - ((ui * ju).sum(1) + (jl * li).sum(1))
            g = -torch.sigmoid(-y)
            loss = torch.nn.functional.softplus(-y).sum() + reg * 0.5 * sum((t * t).sum() for t in (ui, iu, il, li, ju, jl))
            gc = g[:, None]
            G[0].index_add_(0, u, gc * (iu - ju) + reg * ui)
            G[3].index_add_(0, l, gc * (il - jl) + reg * li)
            G[1].index_add_(0, i, gc * ui + reg * iu)
            G[2].index_add_(0, i, gc * li + reg * il)
            G[1].index_add_(0, third, -gc * ui + reg * ju)
            G[2].index_add_(0, third, -gc * li + reg * jl)
        else:
            g = (torch.sigmoid(x) - third) / x.numel()
            loss = torch.nn.functional.binary_cross_entropy_with_logits(x, third) + \
                reg * 0.5 * sum((t * t).sum() for t in (ui, iu, il, li))
            gc = g[:, None]
            G[0].index_add_(0, u, gc * iu + reg * ui)
            G[3].index_add_(0, l, gc * il + reg * li)
            G[1].index_add_(0, i, gc * ui + reg * iu)
            G[2].index_add_(0, i, gc * li + reg * il)
        alpha = lr * (1 - state["b2p"]) ** 0.5 / (1 - state["b1p"])
        for t, gr, m, v in zip(T, G, M, V):                    # TF-1.12's sparse Adam: every row swept
            m.mul_(0.9).add_(gr, alpha=0.1)
            v.mul_(0.999).addcmul_(gr, gr, value=0.001)
            t.addcdiv_(m, v.sqrt().add_(1e-8), value=-alpha)
            gr.zero_()
        state["b1p"] *= 0.9
        state["b2p"] *= 0.999
        return loss
    for k in range(5):
        one(k)
    return _timed(one, len(batches))


def bench_one(a, train, test, ds, d, pairwise):
    import numpy as np
    import torch
    from neurec_amd import engine as E
    from neurec_amd.data import TimeOrderPairwiseSampler, TimeOrderPointwiseSampler
    from neurec_amd.fpmc import FPMCEngine
    from neurec_amd.trainer import FullRankEvaluator
    U, I = train.shape
    rng = np.random.RandomState(2017)
    tabs = [(0.01 * rng.randn(n, d)).astype(np.float32) for n in (U, I, I, I)]
    reg, lr = 0.01, 0.001
    loss = "bpr" if pairwise else "cross_entropy"
    eng = FPMCEngine(*tabs, lr, reg, a.batch, loss=loss, pairwise=pairwise, learner="adam")
    if pairwise:
        sampler = TimeOrderPairwiseSampler(ds, high_order=1, neg_num=1, batch_size=a.batch, shuffle=True,
                                           as_tensors=True)
    else:
        sampler = TimeOrderPointwiseSampler(ds, high_order=1, neg_num=4, batch_size=a.batch, shuffle=True,
                                            as_tensors=True)
    need = a.warmup + a.steps
    batches = []
    while len(batches) < need:
        for bt in sampler:
            if bt[0].numel() == a.batch:
                batches.append(tuple(t.clone() for t in bt))
            if len(batches) == need:
                break
    losses = torch.zeros((need, 2), device="cuda")
    for k in range(a.warmup):
        eng.step(*batches[k], losses[k])
    ms = _timed(lambda k: eng.step(*batches[a.warmup + k], losses[a.warmup + k]), a.steps)
    assert bool(torch.isfinite(losses).all())
    # the split: the C call alone (its rows of G are overwritten by the next call, never applied), then the four
    # applications alone on zero gradients
    grad_ms = _timed(lambda k: eng.gradients(*batches[a.warmup + k], losses[a.warmup + k]), a.steps)
    for g in eng.G.values():
        g.zero_()
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    sweep_bytes = 32 * d * (U + 3 * I)
    last = np.full(U, -1, np.int32)
    for u, s in ds.seqs.items():
        last[u] = s[-1]
    last = torch.from_numpy(last).cuda()
    ranker = FullRankEvaluator(E.DeviceCSR.from_scipy(train), E.DeviceCSR.from_scipy(test), [1, 2, 3, 4, 5], 20)
    users = torch.from_numpy(np.flatnonzero(np.diff(test.indptr) > 0).astype(np.int32)).cuda()
    times = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(6):
        torch.cuda.synchronize()
        e0.record()
        result = ranker.evaluate_factors(eng.user_factors(last), eng.item_factors(), users, exact_mean=True)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    eval_ms = sorted(times[1:])[2]
    dev_batches = [tuple(t.long() if t.dtype == torch.int32 else t for t in bt)
                   for bt in batches[a.warmup:a.warmup + a.torch_steps]]
    torch_ms = _torch_steps(tabs, dev_batches, pairwise, reg, lr) if a.torch_steps else None
    return {"d": d, "mode": "pairwise" if pairwise else "pointwise", "loss": loss, "learner": "adam",
            "num_neg": 1 if pairwise else 4, "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms, 4), "instances_per_s": round(a.batch / (ms * 1e-3), 1),
            "grad_ms": round(grad_ms, 4), "apply_ms": round(apply_ms, 4), "sweep_mbytes_per_step": round(sweep_bytes / 1e6, 2),
            "sweep_gbytes_per_s": round(sweep_bytes / (apply_ms * 1e-3) / 1e9, 1),
            "steps_per_epoch": len(sampler), "eval_width": 2 * d, "eval_users": int(users.numel()),
            "eval_ms": round(eval_ms, 3), "eval_users_per_s": round(users.numel() / (eval_ms * 1e-3), 1),
            "ndcg_at_10": float(np.asarray(result)[3 * 20 + 9]),
            "torch_ms_per_step": None if torch_ms is None else round(torch_ms, 4), "torch_steps": a.torch_steps}


def bench(a):
    from neurec_amd import synth
    train, test = synth.interactions(a.shape)
    train, test = train.tocsr(), test.tocsr()
    train.sort_indices()
    ds = _Dataset(train)
    runs = [bench_one(a, train, test, ds, d, pairwise) for d in (64, 16) for pairwise in (True, False)]
    return {"shape": a.shape, "users": train.shape[0], "items": train.shape[1], "nnz": int(train.nnz), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="gowalla")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--torch-steps", type=int, default=100)
    print(json.dumps(bench(ap.parse_args())), flush=True)


if __name__ == "__main__":
    main()
