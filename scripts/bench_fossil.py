"""Step time and evaluation rate of the Fossil engine (neurec_amd/fossil.py) on the gowalla shape.

    python scripts/bench_fossil.py [--shape gowalla] [--steps 300] [--warmup 30] [--batch 256] [--order 3]
                                   [--torch-steps 100]

The train matrix is the synthetic gowalla-shaped one (neurec_amd/synth.py: the real degree distribution); every user's
time order is a seeded permutation of the row.  The instances come from the device streams of the time-order samplers
at high_order = `--order`, reversed to most-recent-first as the plugin does.  Four configurations: pairwise bpr and
pointwise cross_entropy (num_neg = 4), learner adagrad (conf/Fossil.properties), each at d = 64 and at the reference's
d = 16.  Reported per configuration:

    ms_per_step, instances_per_s   `--steps` engine steps timed between device events, after `--warmup` steps
    grad_ms, apply_ms              the same batches through nrhip_fossil_step alone, and the applications alone (the
                                   dense ones of c1 and eta_bias, the row ones of Q, bias and eta) on the last gradient
    eval_users_per_s               user and item factors at width d + 1 + the full-rank evaluation of every test user
                                   on the factor path (median of 5)
    torch_ms_per_step              the same step in torch eager ops on the same GPU, on histories padded to
                                   [B, Lmax] as the reference feeds them: index_select gathers, index_add_ into dense
                                   gradient buffers, dense Adagrad on c1 / eta_bias and on the touched rows of the
                                   other tables — over `--torch-steps` of the same batches

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


def _torch_steps(tabs, train, batches, pairwise, L, alpha, lr):
    """ms per step of the eager restatement over `batches` (device tuples); regs = 0 as conf/Fossil.properties"""
    import numpy as np
    import torch
    dev = "cuda"
    c1, Q, bias, eta, eb = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in tabs]
    I, d = c1.shape
    deg = np.diff(train.indptr)
    Lmax = int(deg.max())
    pad = np.full((train.shape[0], Lmax), I, np.int64)          # the padded histories, built once: not timed
    for u in range(train.shape[0]):
        pad[u, :deg[u]] = train.indices[train.indptr[u]:train.indptr[u + 1]]
    pad, degt = torch.from_numpy(pad).to(dev), torch.from_numpy(deg.astype(np.float32)).to(dev)
    T = [c1, Q, bias, eta, eb]
    G = [torch.zeros_like(t) for t in T]
    A = [torch.full_like(t, 1e-8) for t in T]

    def side(u, rec, item, excl, n):
        h = pad.index_select(0, u)[:, :int(n.max().item()) + 1]                 # padded to the batch's longest row
        keep = (h != I) & (h != excl[:, None])
        rows = torch.cat([c1, c1.new_zeros(1, d)]).index_select(0, h.reshape(-1)).view(h.shape[0], h.shape[1], d)
        p = (rows * keep[:, :, None]).sum(1)
        w = eb[None, :] + eta.index_select(0, u)
        short = c1.index_select(0, rec.reshape(-1)).view(-1, L, d)
        s = (w[:, :, None] * short).sum(1)
        q = Q.index_select(0, item)
        coeff = n.pow(-alpha)
        out = coeff * (p * q).sum(1) + (s * q).sum(1) + bias.index_select(0, item)
        return out, (h, keep, p, w, short, s, q, coeff)

    def back(u, rec, item, dout, saved):
        h, keep, p, w, short, s, q, coeff = saved
        g = (dout * coeff)[:, None] * q
        G[0].index_add_(0, h.clamp(max=I - 1).reshape(-1), (g[:, None, :] * keep[:, :, None]).reshape(-1, d))
        G[0].index_add_(0, rec.reshape(-1), ((dout[:, None] * w)[:, :, None] * q[:, None, :]).reshape(-1, d))
        G[1].index_add_(0, item, dout[:, None] * (coeff[:, None] * p + s))
        G[2].index_add_(0, item, dout)
        gw = dout[:, None] * (short * q[:, None, :]).sum(2)
        G[3].index_add_(0, u, gw)
        G[4].add_(gw.sum(0))

    def one(k):
        u, rec, item, third = batches[k % len(batches)]
        n = degt.index_select(0, u)
        if pairwise:
            op, sp_ = side(u, rec, item, item, n - 1)
            on, sn = side(u, rec, third, torch.full_like(item, -1), n)
            y = op - on
            loss = torch.nn.functional.softplus(-y).sum()
            dl = -torch.sigmoid(-y)
            back(u, rec, item, dl, sp_)
            back(u, rec, third, -dl, sn)
        else:
            excl = torch.where(third > 0.5, item, torch.full_like(item, -1))
            out, sv = side(u, rec, item, excl, torch.where(third > 0.5, n - 1, n))
            loss = torch.nn.functional.binary_cross_entropy_with_logits(out, third)
            back(u, rec, item, (torch.sigmoid(out) - third) / out.numel(), sv)
        for t, g, a in zip(T, G, A):                           # Adagrad; untouched rows have g = 0 and do not move
            a.addcmul_(g, g)
            t.addcdiv_(g, a.sqrt(), value=-lr)
            g.zero_()
        return loss
    for k in range(5):
        one(k)
    return _timed(one, len(batches))


def bench_one(a, train, test, ds, d, pairwise):
    import numpy as np
    import torch
    from neurec_amd import engine as E
    from neurec_amd.data import TimeOrderPairwiseSampler, TimeOrderPointwiseSampler
    from neurec_amd.fossil import FossilEngine
    from neurec_amd.model.sequential_recommender.Fossil import last_items_table, recents_for_engine
    from neurec_amd.trainer import FullRankEvaluator
    U, I = train.shape
    L = a.order
    rng = np.random.RandomState(2017)
    tabs = [(0.01 * rng.randn(I, d)).astype(np.float32), (0.01 * rng.randn(I, d)).astype(np.float32),
            np.zeros(I, np.float32), (0.01 * rng.randn(U, L)).astype(np.float32),
            (0.01 * rng.randn(L)).astype(np.float32)]
    regs, lr, alpha = (0.0, 0.0, 0.0), 0.001, 0.5
    loss = "bpr" if pairwise else "cross_entropy"
    last = last_items_table(ds.seqs, U, L)
    eng = FossilEngine(tabs[0], tabs[1], tabs[3], tabs[4], train, lr, regs, alpha, a.batch, loss=loss,
                       pairwise=pairwise, learner="adagrad", bias=tabs[2], last_items=last)
    if pairwise:
        sampler = TimeOrderPairwiseSampler(ds, high_order=L, neg_num=1, batch_size=a.batch, shuffle=True,
                                           as_tensors=True)
    else:
        sampler = TimeOrderPointwiseSampler(ds, high_order=L, neg_num=4, batch_size=a.batch, shuffle=True,
                                            as_tensors=True)
    need = a.warmup + a.steps
    batches = []
    while len(batches) < need:
        for u, rec, it, third in sampler:
            if u.numel() == a.batch:
                batches.append((u.clone(), recents_for_engine(rec, L).clone(), it.clone(), third.clone()))
            if len(batches) == need:
                break
    losses = torch.zeros((need, 2), device="cuda")
    for k in range(a.warmup):
        eng.step(*batches[k], losses[k])
    ms = _timed(lambda k: eng.step(*batches[a.warmup + k], losses[a.warmup + k]), a.steps)
    assert bool(torch.isfinite(losses).all())

    # the split: the C call alone (its gradient buffers are overwritten by the next call, never applied), then the
    # applications alone on the last gradient
    grad_ms = _timed(lambda k: eng.gradients(*batches[a.warmup + k], losses[a.warmup + k]), a.steps)
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    ranker = FullRankEvaluator(E.DeviceCSR.from_scipy(train), E.DeviceCSR.from_scipy(test), [1, 2, 3, 4, 5], 20)
    users = torch.from_numpy(np.flatnonzero(np.diff(test.indptr) > 0).astype(np.int32)).cuda()
    times = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(6):
        torch.cuda.synchronize()
        e0.record()
        result = ranker.evaluate_factors(eng.user_factors(eng.last_items), eng.item_factors(), users, exact_mean=True)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    eval_ms = sorted(times[1:])[2]
    torch_ms = None
    if a.torch_steps:
        dev_batches = [tuple(t.long() if t.dtype == torch.int32 else t for t in bt)
                       for bt in batches[a.warmup:a.warmup + a.torch_steps]]
        torch_ms = _torch_steps(tabs, train, dev_batches, pairwise, L, alpha, lr)
    return {"d": d, "mode": "pairwise" if pairwise else "pointwise", "loss": loss, "learner": "adagrad",
            "high_order": L, "num_neg": 1 if pairwise else 4, "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms, 4), "instances_per_s": round(a.batch / (ms * 1e-3), 1),
            "grad_ms": round(grad_ms, 4), "apply_ms": round(apply_ms, 4), "steps_per_epoch": len(sampler),
            "eval_width": d + 1, "eval_users": int(users.numel()), "eval_ms": round(eval_ms, 3),
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
    runs = [bench_one(a, train, test, ds, d, pairwise) for d in (64, 16) for pairwise in (True, False)]
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
