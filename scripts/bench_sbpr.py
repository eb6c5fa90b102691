"""Set build, epoch stream, step and scoring of the SBPR engine (neurec_amd/sbpr.py) on the gowalla shape.

    python scripts/bench_sbpr.py [--shape gowalla] [--steps 300] [--warmup 30] [--batch 512] [--score-users 2048]

The train matrix is the synthetic gowalla-shaped one and the trust graph the synthetic one of neurec_amd/synth.py
(log-normal out-degree, power-law popularity of the trusted, edges to users with train items); the hyper-parameters are
conf/SBPR.properties' (d = 16, B = 512, bpr / adam, reg_mf = 0.01).  Each figure stands beside a torch restatement of
the same work on the same device.  Reported:

    sets        the engine's build of the social sets — sizes, block plan, expansion, sort, compaction, the eligible
                users (median of 5 after one untimed build, wall clock around a synchronised device: the build reads
                its sizes back) against torch: the sparse product S @ R, R's own pattern struck from it by a key
                search
    stream      one sample_epoch() (median of 5, device events) against torch: a permutation, k by randint over the
                set sizes, j by three rounds of rejection against both sets through searchsorted on (user, item) keys
    step        ms_per_step over `--steps` steps of full batches from the device stream, timed between device events
                after `--warmup` steps; grad_ms / apply_ms: nrhip_sbpr_step alone and the three applications alone;
                torch_ms: the eager step — embedding lookups, the loss, autograd and torch.optim.Adam on the three
                tables; traffic_bound_ms: the bytes the step has to move over the 8 TB/s of HBM — Adam's sparse form
                sweeps every entry of P, Q and b (the variable and both moments read and written, the gradient read
                and cleared: 8 floats an entry) plus the batch's row gathers
    score       engine.score() of `--score-users` users against every item (median of 5) against torch.matmul

One JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_fpmc import _timed          # noqa: E402

HBM_BYTES_PER_S = 8.0e12
D, LR, REG = 16, 0.001, 0.01


def _median_ms(fn, events=True, n=5):
    import torch
    times = []
    for k in range(n + 1):
        torch.cuda.synchronize()
        if events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        else:
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times[1:])[n // 2], out


def _engine(train, trust, batch, workspace_pairs):
    import numpy as np
    from neurec_amd.sbpr import SBPREngine
    U, I = train.shape
    rng = np.random.RandomState(2017)
    tabs = [(0.01 * rng.randn(*s)).astype(np.float32) for s in ((U, D), (I, D), (I,))]
    return SBPREngine(*tabs, train, trust, LR, REG, batch, loss="bpr", learner="adam", workspace_pairs=workspace_pairs)


def _torch_csr(m):
    import torch
    return torch.sparse_csr_tensor(torch.from_numpy(m.indptr.astype("int64")), torch.from_numpy(m.indices.astype("int64")),
                                   torch.ones(m.nnz, dtype=torch.float32), size=m.shape).cuda()


def torch_sets(S, R, r_keys, n_items):
    """(user, item) keys and counts of S @ R minus R's own pattern"""
    import torch
    prod = torch.sparse.mm(S, R).to_sparse_coo().coalesce()
    idx = prod.indices()
    keys = idx[0] * n_items + idx[1]
    at = torch.searchsorted(r_keys, keys).clamp_(max=r_keys.numel() - 1)
    keep = r_keys[at] != keys
    return keys[keep], prod.values()[keep]


def torch_stream(eng, r_keys, c_keys, generator):
    """an epoch's five fields the eager way; three rounds of rejection for j (what is still inside a set after them is
    left: the restatement is timed, not used)"""
    import torch
    n, I = eng.n_instances, eng.n_items
    perm = torch.randperm(n, device="cuda", generator=generator)
    row = eng._slot_row.long()[perm]
    u = eng.eligible_users.long()[row]
    i = eng.tr_indices.long()[eng.tr_indptr[u] + (perm - eng._slot_ptr[row])]
    nc = eng.c_indptr[u + 1] - eng.c_indptr[u]
    at = eng.c_indptr[u] + (torch.rand(n, device="cuda", generator=generator) * nc).long().clamp_(max=nc - 1)
    k, suk = eng.c_items.long()[at], (eng.c_counts[at] + 1).float()
    j = torch.randint(I, (n,), device="cuda", generator=generator)
    for _ in range(3):
        key = u * I + j
        bad = (r_keys[torch.searchsorted(r_keys, key).clamp_(max=r_keys.numel() - 1)] == key) | \
              (c_keys[torch.searchsorted(c_keys, key).clamp_(max=c_keys.numel() - 1)] == key)
        j = torch.where(bad, torch.randint(I, (n,), device="cuda", generator=generator), j)
    return u, i, k, j, suk


def torch_step_fn(eng):
    """the eager step: lookups, loss, autograd, Adam on the three tables"""
    import torch
    P, Q, b = (t.clone().requires_grad_(True) for t in (eng.P, eng.Q, eng.b))
    opt = torch.optim.Adam([P, Q, b], lr=LR)

    def step(u, i, k, j, suk):
        u, i, k, j = u.long(), i.long(), k.long(), j.long()
        p = P[u]
        x = lambda a: (p * Q[a]).sum(1) + b[a]
        xi, xk, xj = x(i), x(k), x(j)
        loss = -torch.nn.functional.logsigmoid((xi - xk) / suk).sum() - torch.nn.functional.logsigmoid(xk - xj).sum()
        loss = loss + REG * 0.5 * (p.pow(2).sum() + sum(Q[a].pow(2).sum() + b[a].pow(2).sum() for a in (i, k, j)))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return step


def bench(a):
    import numpy as np
    import torch
    from neurec_amd import synth
    train, test = synth.interactions(a.shape)
    train = train.tocsr()
    train.sort_indices()
    U, I = train.shape
    trust = synth.trust_graph(U, has_items=np.diff(train.indptr) > 0)
    out = {"script": "scripts/bench_sbpr.py", "shape": a.shape, "users": U, "items": I, "nnz": int(train.nnz),
           "trust_edges": int(trust.nnz), "d": D, "batch": a.batch}

    # ---- sets
    eng = _engine(train, trust, a.batch, a.workspace_pairs)
    sets_ms, _ = _median_ms(eng._build_sets, events=False)
    S, R = _torch_csr(trust), _torch_csr(train)
    r_keys = (torch.repeat_interleave(torch.arange(U, device="cuda"), eng.tr_indptr[1:] - eng.tr_indptr[:-1]) * I
              + eng.tr_indices.long())
    torch_sets_ms, (c_keys, c_vals) = _median_ms(lambda: torch_sets(S, R, r_keys, I), events=False)
    own = torch.repeat_interleave(torch.arange(U, device="cuda"), eng.c_indptr[1:] - eng.c_indptr[:-1]) * I \
        + eng.c_items.long()
    has = (eng.tr_indptr[1:] > eng.tr_indptr[:-1])[c_keys // I]           # train_dict holds users with train items only
    assert torch.equal(c_keys[has], own) and torch.equal(c_vals[has].int(), eng.c_counts)
    out["sets"] = {"expanded_pairs": int(sum(n for _, _, n in eng.blocks)), "blocks": eng.n_blocks,
                   "social_entries": int(eng.c_items.numel()), "eligible_users": int(eng.eligible_users.numel()),
                   "build_ms": round(sets_ms, 3), "torch_ms": round(torch_sets_ms, 3),
                   "torch_over_engine": round(torch_sets_ms / sets_ms, 2)}

    # ---- stream
    epoch = [0]

    def draw():
        epoch[0] += 1
        return eng.sample_epoch(epoch[0])
    stream_ms, fields = _median_ms(draw)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    torch_stream_ms, _ = _median_ms(lambda: torch_stream(eng, r_keys, own, gen))
    out["stream"] = {"instances": eng.n_instances, "epoch_ms": round(stream_ms, 4),
                     "instances_per_s": round(eng.n_instances / (stream_ms * 1e-3), 1),
                     "torch_ms": round(torch_stream_ms, 3), "torch_over_engine": round(torch_stream_ms / stream_ms, 2)}

    # ---- step
    B, need = a.batch, a.warmup + a.steps
    batches = []
    while len(batches) < need:
        f = draw()
        for lo in range(0, eng.n_instances - B + 1, B):
            batches.append(tuple(x[lo:lo + B] for x in f))
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
    tstep = torch_step_fn(eng)
    for k in range(a.warmup):
        tstep(*batches[k])
    torch_ms = _timed(lambda k: tstep(*batches[a.warmup + k]), a.steps)
    # Adam's sparse form sweeps every row: var, m, v read and written, the gradient read and cleared = 8 floats per
    # entry of P, Q and b; the batch's gathers: 4 rows of d floats read by the forward pass, again by the rows kernel
    entries = U * D + I * D + I
    traffic = 4.0 * (8 * entries + 2 * 4 * B * D)
    bound_ms = traffic / HBM_BYTES_PER_S * 1e3
    out["step"] = {"steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 4),
                   "instances_per_s": round(B / (ms * 1e-3), 1), "grad_ms": round(grad_ms, 4),
                   "apply_ms": round(apply_ms, 4), "torch_ms": round(torch_ms, 4),
                   "torch_over_engine": round(torch_ms / ms, 2), "traffic_bytes": int(traffic),
                   "traffic_bound_ms": round(bound_ms, 5), "step_over_traffic_bound": round(ms / bound_ms, 1),
                   "steps_per_epoch": (eng.n_instances + B - 1) // B}

    # ---- score
    users = torch.from_numpy(np.flatnonzero(np.diff(test.tocsr().indptr) > 0).astype(np.int32)[:a.score_users]).cuda()
    score_ms, Sc = _median_ms(lambda: eng.score(users))
    torch_score_ms, St = _median_ms(lambda: eng.P[users.long()] @ eng.Q.T)
    assert float((Sc - St).abs().max()) <= 1e-4 * float(St.abs().max())
    n = int(users.numel())
    out["score"] = {"score_users": n, "score_ms": round(score_ms, 4), "pairs_per_s": round(n * I / (score_ms * 1e-3), 1),
                    "torch_ms": round(torch_score_ms, 4), "torch_over_engine": round(torch_score_ms / score_ms, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="gowalla")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--score-users", type=int, default=2048)
    ap.add_argument("--workspace-pairs", type=int, default=1 << 23)
    print(json.dumps(bench(ap.parse_args())), flush=True)


if __name__ == "__main__":
    main()
