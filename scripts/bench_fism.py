"""Step time and evaluation rate of the FISM engine (neurec_amd/fism.py) on the gowalla shape, shipped config.

    python scripts/bench_fism.py [--shape gowalla] [--steps 2000] [--warmup 200] [--batch 256] [--d 16]
                                 [--torch-steps 50] [--learner adam]

The train matrix is the synthetic gowalla-shaped one (neurec_amd/synth.py); the instances come from the device stream
(PointwiseSampler, num_neg = 4), square loss, adam: conf/FISM.properties as shipped.  Reported:

    ms_per_step, instances_per_s   `--steps` engine steps timed between device events, after `--warmup` steps
    eval_users_per_s               user factors of every user + the full-rank evaluation of every test user on the
                                   factor path (median of 5)
    torch_ms_per_step              for scale: the reference's formulation restated in plain torch on the device — the
                                   batch padded to [B, Lmax] on the host beforehand (not timed), `c1` with a zero pad
                                   row gathered to [B, Lmax, d], autograd, torch.optim.Adam on the three tables — over
                                   `--torch-steps` of the same batches
    history_rows_per_step          mean over the timed steps of sum_b |H_b|: the c1 rows one step gathers and scatters

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
    """what the samplers ask of data.dataset.Dataset"""

    def __init__(self, train):
        self.train_matrix = train
        self.num_users, self.num_items = train.shape

    def get_user_train_dict(self, by_time=False):
        m = self.train_matrix
        return {u: m.indices[m.indptr[u]:m.indptr[u + 1]].tolist() for u in range(m.shape[0])
                if m.indptr[u + 1] > m.indptr[u]}


def _torch_steps(train, c1, Q, batches, alpha, regs, lr):
    """ms per step of the padded-gather + autograd restatement over `batches` (host tuples)"""
    import numpy as np
    import torch
    I, d = c1.shape
    dev = "cuda"
    c1 = torch.nn.Parameter(torch.from_numpy(c1).to(dev))
    Q = torch.nn.Parameter(torch.from_numpy(Q).to(dev))
    bias = torch.nn.Parameter(torch.zeros(I, device=dev))
    opt = torch.optim.Adam([c1, Q, bias], lr=lr)
    deg = np.diff(train.indptr)
    feeds = []
    for users, items, labels in batches:
        L = int(deg[users].max())
        H = np.full((len(users), max(L, 1)), I, np.int64)
        n = np.empty(len(users), np.float32)
        for k, (u, i, y) in enumerate(zip(users, items, labels)):
            row = train.indices[train.indptr[u]:train.indptr[u + 1]]
            if y > 0.5:
                row = row[row != i]
            H[k, :len(row)] = row
            n[k] = len(row) + 1
        feeds.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                           for a in (H, n, items.astype(np.int64), labels)))
    pad = torch.zeros((1, d), device=dev)

    def one(H, n, items, labels):
        p = torch.cat([c1, pad], 0)[H].sum(1)
        q = Q[items]
        out = n.pow(-alpha) * (p * q).sum(1) + bias[items]
        loss = ((labels - out) ** 2).sum() + regs[0] * 0.5 * (p * p).sum() + regs[1] * 0.5 * (q * q).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    for f in feeds[:5]:
        one(*f)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for f in feeds:
        one(*f)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / len(feeds)


def bench(a):
    import numpy as np
    import torch
    from neurec_amd import engine as E
    from neurec_amd import synth
    from neurec_amd.data import PointwiseSampler
    from neurec_amd.fism import FISMEngine
    from neurec_amd.trainer import FullRankEvaluator
    train, test = synth.interactions(a.shape)
    train = train.tocsr()
    train.sort_indices()
    U, I = train.shape
    rng = np.random.RandomState(2017)
    c1 = (0.01 * rng.randn(I, a.d)).astype(np.float32)
    Q = (0.01 * rng.randn(I, a.d)).astype(np.float32)
    alpha, regs, lr = 0.5, [1e-7, 1e-7], 0.001
    eng = FISMEngine(c1, Q, train, lr, regs, alpha, a.batch, loss="square", pairwise=False, learner=a.learner)
    sampler = PointwiseSampler(_Dataset(train), neg_num=4, batch_size=a.batch, shuffle=True, as_tensors=True)
    need = a.warmup + a.steps
    batches = []
    while len(batches) < need:
        for bt in sampler:
            if bt[0].numel() == a.batch:
                batches.append(bt)
            if len(batches) == need:
                break
    losses = torch.zeros((need, 2), device="cuda")
    for k in range(a.warmup):
        eng.step(*batches[k], losses[k])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(a.warmup, need):
        eng.step(*batches[k], losses[k])
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    assert bool(torch.isfinite(losses).all())
    deg = np.diff(train.indptr)
    hist = float(np.mean([deg[bt[0].cpu().numpy()].sum() for bt in batches[a.warmup:a.warmup + 50]]))
    # evaluation: user factors of every user, then the factor path over every test user
    test = test.tocsr()
    ranker = FullRankEvaluator(E.DeviceCSR.from_scipy(train), E.DeviceCSR.from_scipy(test), [1, 2, 3, 4, 5], 20)
    users = torch.from_numpy(np.flatnonzero(np.diff(test.indptr) > 0).astype(np.int32)).cuda()
    times = []
    for _ in range(6):
        torch.cuda.synchronize()
        e0.record()
        P = eng.user_factors()
        result = ranker.evaluate_factors(P, eng.item_factors(), users, exact_mean=True)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    eval_ms = sorted(times[1:])[2]
    host = [tuple(t.cpu().numpy() for t in bt) for bt in batches[a.warmup:a.warmup + a.torch_steps]]
    torch_ms = _torch_steps(train, c1, Q, host, alpha, regs, lr) if a.torch_steps else None
    return {"shape": a.shape, "users": U, "items": I, "nnz": int(train.nnz), "d": a.d, "batch": a.batch, "num_neg": 4,
            "loss": "square", "learner": a.learner, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms, 4), "instances_per_s": round(a.batch / (ms * 1e-3), 1),
            "steps_per_epoch": int(-(-train.nnz * 5 // a.batch)), "history_rows_per_step": round(hist, 1),
            "eval_users": int(users.numel()), "eval_ms": round(eval_ms, 3),
            "eval_users_per_s": round(users.numel() / (eval_ms * 1e-3), 1), "ndcg_at_10": float(np.asarray(result)[3 * 20 + 9]),
            "torch_ms_per_step": None if torch_ms is None else round(torch_ms, 4), "torch_steps": a.torch_steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="gowalla")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--torch-steps", type=int, default=50)
    ap.add_argument("--learner", default="adam")
    print(json.dumps(bench(ap.parse_args())), flush=True)


if __name__ == "__main__":
    main()
