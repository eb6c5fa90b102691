"""Step time of the GRU4RecPlus engine (neurec_amd/gru4recplus.py) at the reference's defaults, beside GRU4Rec's step
at the same batch and layers, on the gowalla shape.

    python scripts/bench_gru4recplus.py [--shape gowalla] [--steps 200] [--warmup 30] [--repeats 5] [--batch 256]
                                        [--n-sample 2048]

The train matrix is the synthetic gowalla-shaped one (neurec_amd/synth.py); every user's time order is a seeded
permutation of the row; the feeds are the plugin's own (`epoch_feeds`: the session-parallel schedule and the
popularity sampler).  layers [100], bpr_max / tanh / linear (conf/GRU4RecPlus.properties); GRU4Rec: top1 / tanh / linear
(conf/GRU4Rec.properties).  In ONE process, the two engines in turn, `--repeats` windows of `--steps` steps each, timed
between device events after `--warmup` steps: the median window and the range, in ms per step.

    plus            ms_per_step (median, min, max), grad_ms / apply_ms (nrhip_gru4recplus_step alone and the Adam
                    applications alone: launch-bound loops, not a split)
    gru4rec         the same for GRU4Rec's step at the same B and layers
    block_cost_ms   plus - gru4rec, medians: what the B x (B + n_sample) block costs over the B x B one
    bound           the three products of the block (Z, dZ Qy, dZ^T h_top): 3 B M n multiply-adds over VALU_RATE (the
                    unpacked fp32 issue rate of the VALU, a quarter of the 157.3 TFLOP/s vector peak), and the bytes they
                    must move once (Z and dZ written, Z read once and dZ twice, Qy read three times, sQ written) over
                    the measured 6.29 TB/s HBM copy rate — an upper estimate of the traffic, since 12 MB sit in L2 /
                    Infinity Cache; bound_ms is the larger; block_cost_over_bound = block_cost_ms / bound_ms

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
from bench_gru4rec import LAYERS, VALU_RATE, _engine          # noqa: E402

HBM_RATE = 6.29e12
SAMPLE_ALPHA = 0.75


def _plus_engine(n_items, batch, n_sample):
    import numpy as np
    from neurec_amd.gru4recplus import GRU4RecPlusEngine
    from neurec_amd.util.tool import get_initializer
    embed, kernel = get_initializer("tnormal", 0.01, seed=2017), get_initializer("xavier_uniform", 0.01, seed=2018)
    cells, n_in = [], LAYERS[0]
    for n in LAYERS:
        cells.append((kernel([n_in + n, 2 * n]), np.ones(2 * n, np.float32), kernel([n_in + n, n]),
                      np.zeros(n, np.float32)))
        n_in = n
    return GRU4RecPlusEngine(embed([n_items, LAYERS[0]]), embed([n_items, LAYERS[-1]]), np.zeros(n_items, np.float32),
                             cells, 0.01, 0.0, batch, loss="bpr_max", hidden_act="tanh", final_act="linear",
                             bpr_reg=1.0, n_sample=n_sample)


def _windows(eng, X, Y, reset, losses, a):
    """(sorted window times in ms per step, grad_ms, apply_ms)"""
    import torch
    for k in range(a.warmup):
        eng.step(X[k], Y[k], losses[k], reset[k])
    times = []
    for r in range(a.repeats):
        w = a.warmup + r * a.steps
        times.append(_timed(lambda k: eng.step(X[w + k], Y[w + k], losses[w + k], reset[w + k]), a.steps))
    assert bool(torch.isfinite(losses).all())
    w = a.warmup
    grad_ms = _timed(lambda k: eng.gradients(X[w + k], Y[w + k], losses[w + k]), a.steps)
    for g in eng.G.values():
        g.zero_()
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    return sorted(times), grad_ms, apply_ms


def _report(times, grad_ms, apply_ms):
    return {"ms_per_step": round(times[len(times) // 2], 4), "min": round(times[0], 4), "max": round(times[-1], 4),
            "windows": [round(t, 4) for t in times], "grad_ms": round(grad_ms, 4), "apply_ms": round(apply_ms, 4)}


def bench(a):
    import numpy as np
    import torch
    from neurec_amd import synth
    from neurec_amd.model.sequential_recommender.GRU4RecPlus import epoch_feeds, popularity_cumsum
    train, _ = synth.interactions(a.shape)
    train = train.tocsr()
    train.sort_indices()
    ds = _Dataset(train)
    U, I = train.shape
    lens = np.zeros(U, np.int64)
    for u, s in ds.seqs.items():
        lens[u] = len(s)
    seq_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seq = np.asarray([i for u in range(U) for i in ds.seqs.get(u, [])], np.int32)
    present = np.flatnonzero(lens > 0)
    offset = np.concatenate([seq_ptr[present], [seq_ptr[-1]]])
    np.random.seed(7)
    X, Y, reset = epoch_feeds(offset, seq, popularity_cumsum(seq, SAMPLE_ALPHA), a.batch, a.n_sample)
    need, per_epoch = a.warmup + a.repeats * a.steps, len(X)
    assert per_epoch >= need, (per_epoch, need)
    dev = torch.device("cuda")
    X, Y, reset = (torch.from_numpy(t[:need]).to(dev) for t in (X, Y, reset))
    B, M, n = a.batch, a.batch + a.n_sample, LAYERS[-1]
    out = {"script": "scripts/bench_gru4recplus.py", "shape": a.shape, "users": U, "items": I, "layers": LAYERS,
           "batch": B, "n_sample": a.n_sample, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "steps_per_epoch": per_epoch}
    plus = _plus_engine(I, B, a.n_sample)
    out["plus"] = _report(*_windows(plus, X, Y, reset, torch.zeros((need, 2), device=dev), a))
    del plus
    base = _engine(I, B)
    Yb = Y[:, :B].contiguous()
    out["gru4rec"] = _report(*_windows(base, X, Yb, reset, torch.zeros((need, 2), device=dev), a))
    fma = 3 * B * M * n
    moved = 4 * (5 * B * M + 3 * M * n + M * n + 2 * B * n)
    bound = max(fma / VALU_RATE, moved / HBM_RATE) * 1e3
    cost = out["plus"]["ms_per_step"] - out["gru4rec"]["ms_per_step"]
    out.update(block_cost_ms=round(cost, 4), products_fma=fma, products_bytes=moved,
               bound_fma_ms=round(fma / VALU_RATE * 1e3, 5), bound_bytes_ms=round(moved / HBM_RATE * 1e3, 5),
               bound_ms=round(bound, 5), block_cost_over_bound=round(cost / bound, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="gowalla")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n-sample", type=int, default=2048)
    print(json.dumps(bench(ap.parse_args())), flush=True)


if __name__ == "__main__":
    main()
