"""Pairs, block step, optimiser sweep and scoring of the JCA engine (neurec_amd/jca.py) on the gowalla shape.

    python scripts/bench_jca.py [--shape gowalla] [--steps 200] [--warmup 20] [--batch 256] [--score-users 2048]

The train matrix is the synthetic gowalla-shaped one of neurec_amd/synth.py; the hyper-parameters are
conf/JCA.properties' (H = 50, B = 256, tanh / tanh, adam, reg = 0, margin 0.15, num_neg = 1).  The blocks are those of an
epoch: a permutation of the users and of the items cut into batches.  Each figure stands beside an eager torch
restatement of the same work on the same device (which feeds dense slabs cut from a uint8 copy of the matrix, as the
reference feeds them from its `toarray()`) and beside its traffic bound.  Reported:

    pairs       engine.pairs() of one block (`ms_per_block`, over `--steps` blocks between device events, the 4-byte
                read of the count included) and pairs per second; torch: the block's sub-matrix, its positives by
                nonzero(), a negative each by three rounds of rejection
    step        engine.step() of one block from its pairs: ms_per_step; grad_ms / apply_ms: nrhip_jca_step alone and
                the sweep alone; torch: slabs, both encoders, the decoders on the block's columns, the hinge, autograd
                and torch.optim.Adam over the nine dense variables
    apply       the sweep alone against torch.optim.Adam's step alone; its bound is the Adam traffic: the variable and
                both moments read and written, 6 floats per entry of 2 (U + I) H + 2 I + U + 2 H
    score       engine.score() of `--score-users` users against every item, item codes ready (median of 5), against
                torch on the dense slab; the bound is the [n, I] output written once

`*_over_bound` is the measured time over the traffic bound at 8 TB/s.  One JSON line.
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
from bench_sbpr import _median_ms      # noqa: E402

HBM_BYTES_PER_S = 8.0e12
H, LR, MARGIN, NUM_NEG = 50, 0.001, 0.15, 1


def _blocks(U, I, B, need, seed=7):
    import numpy as np
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < need:
        pu, pi = rs.permutation(U), rs.permutation(I)
        for i in range(U // B):
            for j in range(I // B):
                out.append((pu[i * B:(i + 1) * B].astype(np.int32), pi[j * B:(j + 1) * B].astype(np.int32), i, j))
                if len(out) == need:
                    return out
    return out


def torch_pairs(Rd, rows, cols, generator):
    import torch
    sub = Rd[rows][:, cols]
    a, bp = torch.nonzero(sub, as_tuple=True)
    bn = torch.randint(cols.numel(), a.shape, device="cuda", generator=generator)
    for _ in range(3):
        bn = torch.where(sub[a, bn] != 0, torch.randint(cols.numel(), a.shape, device="cuda", generator=generator), bn)
    return a, bp, bn


def torch_model(tables):
    import torch
    T = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in tables.items()}
    return T, torch.optim.Adam(list(T.values()), lr=LR)


def torch_forward(T, Ru, Ri, rows, cols):
    import torch
    hu = torch.tanh(Ru @ T["UV"] + T["Ub1"])
    hi = torch.tanh((Ri.t() @ T["IV"] + T["Ib1"]) * T["I_factor_vector"][0, cols][:, None])
    xu = hu @ T["UW"][:, cols] + T["Ub2"][0, cols]
    xi = (hi @ T["IW"][:, rows] + T["Ib2"][0, rows]).t()
    return (torch.tanh(xu) + torch.tanh(xi)) / 2.0


def bench(a):
    import numpy as np
    import torch
    from neurec_amd import synth
    from neurec_amd.jca import JCAEngine
    from neurec_amd.model.general_recommender.JCA import initial_variables
    train, test = synth.interactions(a.shape)
    train = train.tocsr()
    train.sort_indices()
    train.data[:] = 1
    U, I = train.shape
    B, need = a.batch, a.warmup + a.steps
    out = {"script": "scripts/bench_jca.py", "shape": a.shape, "users": U, "items": I, "nnz": int(train.nnz), "H": H,
           "batch": B, "blocks_per_epoch": (U // B + 1) * (I // B + 1)}
    tables = initial_variables(U, I, H)
    eng = JCAEngine(tables, train, H, B, num_neg=NUM_NEG, learning_rate=LR, margin=MARGIN)
    blocks = _blocks(U, I, B, need)
    Rd = torch.zeros((U, I), dtype=torch.uint8, device="cuda")
    coo = train.tocoo()
    Rd[torch.from_numpy(coo.row.astype(np.int64)).cuda(), torch.from_numpy(coo.col.astype(np.int64)).cuda()] = 1
    d_blocks = [(torch.from_numpy(r.astype(np.int64)).cuda(), torch.from_numpy(c.astype(np.int64)).cuda())
                for r, c, _, _ in blocks]
    entries = 2 * (U + I) * H + 2 * I + U + 2 * H

    # ---- pairs
    made = [eng.pairs(r, c, 1, i, j) for r, c, i, j in blocks[:a.warmup]]
    pairs_ms = _timed(lambda k: made.append(eng.pairs(*blocks[a.warmup + k][:2], 1, *blocks[a.warmup + k][2:])), a.steps)
    n_pairs = float(np.mean([p.n for p in made]))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    for k in range(a.warmup):
        torch_pairs(Rd, *d_blocks[k], gen)
    torch_pairs_ms = _timed(lambda k: torch_pairs(Rd, *d_blocks[a.warmup + k], gen), a.steps)
    row_nnz = float(np.mean([np.diff(train.indptr)[r].sum() for r, _, _, _ in blocks]))
    pairs_bytes = 12.0 * row_nnz + 8.0 * B + 4.0 * n_pairs + 2 * 64.0 * B
    out["pairs"] = {"pairs_per_block": round(n_pairs, 1), "ms_per_block": round(pairs_ms, 4),
                    "pairs_per_s": round(n_pairs / (pairs_ms * 1e-3), 1), "torch_ms": round(torch_pairs_ms, 4),
                    "torch_over_engine": round(torch_pairs_ms / pairs_ms, 2), "traffic_bytes": int(pairs_bytes),
                    "over_bound": round(pairs_ms / (pairs_bytes / HBM_BYTES_PER_S * 1e3), 1)}

    # ---- step
    losses = torch.zeros((need, 2), device="cuda")
    run = lambda k: eng.step(blocks[k][0], blocks[k][1], made[k], losses[k])
    for k in range(a.warmup):
        run(k)
    step_ms = _timed(lambda k: run(a.warmup + k), a.steps)
    assert bool(torch.isfinite(losses).all()) and float(losses[:, 0].max()) > 0
    grad_ms = _timed(lambda k: eng.gradients(blocks[a.warmup + k][0], blocks[a.warmup + k][1], made[a.warmup + k],
                                             losses[a.warmup + k]), a.steps)
    eng.G.zero_()
    eng.flag.zero_()
    apply_ms = _timed(lambda k: eng.apply(losses[0]), a.steps)

    T, opt = torch_model(tables)

    def tstep(k):
        rows, cols = d_blocks[k]
        Ru, Ri = Rd[rows].float(), Rd[:, cols].float()
        D = torch_forward(T, Ru, Ri, rows, cols)
        pa, pp, pn = (torch.from_numpy(x).cuda() for x in made[k].numpy())
        loss = torch.clamp(D[pa, pn] - D[pa, pp] + MARGIN, min=0).sum()
        opt.zero_grad(set_to_none=False)
        loss.backward()
        opt.step()
    keep = [k for k in range(need) if made[k].n > 0]
    for k in keep[:a.warmup]:
        tstep(k)
    torch_step_ms = _timed(lambda k: tstep(keep[a.warmup + k] if a.warmup + k < len(keep) else keep[-1]), a.steps)
    torch_apply_ms = _timed(lambda k: opt.step(), a.steps)
    apply_bytes = 4.0 * 6 * entries
    step_bytes = apply_bytes + 2 * 12.0 * train.nnz + 4.0 * (5 * B * H + 4 * B * B)
    out["step"] = {"steps": a.steps, "warmup": a.warmup, "ms_per_step": round(step_ms, 4), "grad_ms": round(grad_ms, 4),
                   "torch_ms": round(torch_step_ms, 4), "torch_over_engine": round(torch_step_ms / step_ms, 2),
                   "traffic_bytes": int(step_bytes), "traffic_bound_ms": round(step_bytes / HBM_BYTES_PER_S * 1e3, 5),
                   "over_bound": round(step_ms / (step_bytes / HBM_BYTES_PER_S * 1e3), 1)}
    out["apply"] = {"entries": entries, "ms": round(apply_ms, 4), "torch_ms": round(torch_apply_ms, 4),
                    "torch_over_engine": round(torch_apply_ms / apply_ms, 2), "traffic_bytes": int(apply_bytes),
                    "traffic_bound_ms": round(apply_bytes / HBM_BYTES_PER_S * 1e3, 5),
                    "over_bound": round(apply_ms / (apply_bytes / HBM_BYTES_PER_S * 1e3), 1)}

    # ---- score
    users = np.flatnonzero(np.diff(test.tocsr().indptr) > 0).astype(np.int32)[:a.score_users]
    eng.encode_items()
    score_ms, Sc = _median_ms(lambda: eng.score(users))
    Tn = {k: torch.from_numpy(v).cuda() for k, v in eng.tables().items()}
    d_users = torch.from_numpy(users.astype(np.int64)).cuda()
    all_items = torch.arange(I, device="cuda")
    hi = eng.hi

    def tscore():
        hu = torch.tanh(Rd[d_users].float() @ Tn["UV"] + Tn["Ub1"])
        xu = hu @ Tn["UW"] + Tn["Ub2"]
        xi = (hi @ Tn["IW"][:, d_users] + Tn["Ib2"][0, d_users]).t()
        return (torch.tanh(xu) + torch.tanh(xi)) / 2.0
    torch_score_ms, St = _median_ms(tscore)
    assert float((Sc - St).abs().max()) <= 1e-4 * max(1.0, float(St.abs().max())) and all_items.numel() == I
    n = int(users.size)
    score_bytes = 4.0 * (n * I + 2 * I * H + 2 * n * H)
    out["score"] = {"score_users": n, "score_ms": round(score_ms, 4), "cells_per_s": round(n * I / (score_ms * 1e-3), 1),
                    "torch_ms": round(torch_score_ms, 4), "torch_over_engine": round(torch_score_ms / score_ms, 2),
                    "traffic_bytes": int(score_bytes), "traffic_bound_ms": round(score_bytes / HBM_BYTES_PER_S * 1e3, 5),
                    "over_bound": round(score_ms / (score_bytes / HBM_BYTES_PER_S * 1e3), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="gowalla")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--score-users", type=int, default=2048)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    line = json.dumps(bench(ap.parse_args()))
    args = ap.parse_args()
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
