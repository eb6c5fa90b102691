"""Step time, sequence-kernel time and scoring rate of the GRU4Rec engine (neurec_amd/gru4rec.py) on the gowalla shape.

    python scripts/bench_gru4rec.py [--shape gowalla] [--steps 300] [--warmup 30] [--batch 256] [--score-users 2048]

The train matrix is the synthetic gowalla-shaped one (neurec_amd/synth.py: the real degree distribution); every user's
time order is a seeded permutation of the row.  layers [100], top1 / tanh (conf/GRU4Rec.properties).  Reported, each
beside the bound it is to be read against — the kernels are chains of unpacked fp32 multiply-adds on the VALU, so the
bound is the count of multiply-adds over VALU_RATE lane-instructions per second (a quarter of the 157.3 TFLOP/s vector
peak, which counts a packed multiply-add as four):

    step         B = `--batch`: ms_per_step over `--steps` steps of the session-parallel schedule of one epoch, timed
                 between device events after `--warmup` steps; grad_ms / apply_ms: nrhip_gru4rec_step alone and the
                 Adam applications alone (launch-bound loops, not a split); fma and valu_bound_ms of one step
    user_states  every user's train sequence through the stack (median of 5 after one untimed call): ms; the throughput
                 bound (the multiply-adds of all positions over VALU_RATE); the SERIAL bound — the longest sequence
                 alone, one workgroup, whose time is `longest x per-position latency`, which no tiling of users can
                 beat; the fraction of each reached
    score        final_act leaky_relu: engine.score() of `--score-users` users against every item (median of 5): ms,
                 pairs/s, n I d multiply-adds and the fraction of that bound

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
LAYERS = [100]


def _engine(n_items, batch, final_act="linear"):
    import numpy as np
    from neurec_amd.gru4rec import GRU4RecEngine
    from neurec_amd.util.tool import get_initializer
    embed, kernel = get_initializer("tnormal", 0.01, seed=2017), get_initializer("xavier_uniform", 0.01, seed=2018)
    cells, n_in = [], LAYERS[0]
    for n in LAYERS:
        cells.append((kernel([n_in + n, 2 * n]), np.ones(2 * n, np.float32), kernel([n_in + n, n]),
                      np.zeros(n, np.float32)))
        n_in = n
    return GRU4RecEngine(embed([n_items, LAYERS[0]]), embed([n_items, LAYERS[-1]]), np.zeros(n_items, np.float32), cells,
                         0.0001, 0.0, batch, loss="top1", hidden_act="tanh", final_act=final_act)


def _median5(fn):
    import torch
    times = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(6):
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times[1:])[2], out


def step_fma(B):
    """multiply-adds of one step: forward, the B x B logits and their two backward products, the cell backward"""
    total, n_in = 0, LAYERS[0]
    for n in LAYERS:
        k = n_in + n
        total += B * k * 3 * n              # gates and candidate
        total += B * n * n + B * n_in * 3 * n + (k + 1) * 3 * n * B      # d(r s), dx, the weight gradients
        n_in = n
    return total + 3 * B * B * LAYERS[-1]


def bench_step(a, seq_ptr, seq, n_items):
    import numpy as np
    import torch
    from neurec_amd.model.sequential_recommender.GRU4Rec import session_parallel_schedule
    present = np.flatnonzero(np.diff(seq_ptr) > 0)
    offset = np.concatenate([seq_ptr[present], [seq_ptr[-1]]])
    rs = np.random.RandomState(7)
    X, Y, reset = session_parallel_schedule(offset, rs.permutation(len(present)), a.batch, seq)
    need, per_epoch = a.warmup + a.steps, len(X)
    assert per_epoch >= need, (per_epoch, need)
    eng = _engine(n_items, a.batch)
    dev = eng.E_in.device
    X, Y = torch.from_numpy(X[:need]).to(dev), torch.from_numpy(Y[:need]).to(dev)
    reset = torch.from_numpy(reset[:need]).to(dev)
    losses = torch.zeros((need, 2), device=dev)
    for k in range(a.warmup):
        eng.step(X[k], Y[k], losses[k], reset[k])
    w = a.warmup
    ms = _timed(lambda k: eng.step(X[w + k], Y[w + k], losses[w + k], reset[w + k]), a.steps)
    assert bool(torch.isfinite(losses).all())
    grad_ms = _timed(lambda k: eng.gradients(X[w + k], Y[w + k], losses[w + k]), a.steps)
    for g in eng.G.values():
        g.zero_()
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    fma = step_fma(a.batch)
    bound = fma / VALU_RATE * 1e3
    return {"layers": LAYERS, "loss": "top1", "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
            "steps_per_epoch": per_epoch, "ms_per_step": round(ms, 4),
            "grad_ms": round(grad_ms, 4), "apply_ms": round(apply_ms, 4), "fma": fma,
            "valu_bound_ms": round(bound, 5), "fraction_of_valu_bound": round(bound / ms, 4)}


def bench_user_states(seq_ptr, seq, n_items):
    import numpy as np
    import torch
    eng = _engine(n_items, 1)
    eng.set_sequences(seq_ptr, seq)
    lens = np.diff(seq_ptr)
    ms, H = _median5(lambda: eng.user_states())
    assert bool(torch.isfinite(H).all())
    longest = int(np.argmax(lens))
    serial_ms, _ = _median5(lambda: eng.user_states([longest]))
    n_in, per_pos = LAYERS[0], 0
    for n in LAYERS:
        per_pos += (n_in + n) * 3 * n
        n_in = n
    fma = int(lens.sum()) * per_pos
    bound = fma / VALU_RATE * 1e3
    tiles = -(-len(lens) // 16)
    order = np.sort(lens)[::-1]
    tile_positions = int(order[::16].sum())
    return {"layers": LAYERS, "users": int(len(lens)), "positions": int(lens.sum()), "longest": int(lens.max()),
            "tiles": tiles, "tile_positions": tile_positions, "ms": round(ms, 3), "fma": fma,
            "valu_bound_ms": round(bound, 4), "fraction_of_valu_bound": round(bound / ms, 4),
            "serial_bound_ms": round(serial_ms, 3), "per_position_us": round(serial_ms * 1e3 / max(int(lens.max()), 1), 3),
            "fraction_of_serial_bound": round(serial_ms / ms, 4)}


def bench_score(a, seq_ptr, seq, n_items):
    import numpy as np
    import torch
    eng = _engine(n_items, 1, final_act="leaky_relu")
    eng.set_sequences(seq_ptr, seq)
    eng.user_states()
    users = np.flatnonzero(np.diff(seq_ptr) > 0)[:a.score_users]
    ms, S = _median5(lambda: eng.score(users))
    assert bool(torch.isfinite(S).all())
    n, d = len(users), LAYERS[-1]
    bound = n * n_items * d / VALU_RATE * 1e3
    return {"final_act": "leaky_relu", "d": d, "score_users": n, "items": n_items, "score_ms": round(ms, 3),
            "score_pairs_per_s": round(n * n_items / (ms * 1e-3), 1), "fma": n * n_items * d,
            "valu_bound_ms": round(bound, 4), "fraction_of_valu_bound": round(bound / ms, 3)}


def bench(a):
    import numpy as np
    from neurec_amd import synth
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
    return {"script": "scripts/bench_gru4rec.py", "shape": a.shape, "users": U, "items": I, "nnz": int(train.nnz),
           "step": bench_step(a, seq_ptr, seq, I), "user_states": bench_user_states(seq_ptr, seq, I),
           "score": bench_score(a, seq_ptr, seq, I)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="gowalla")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--score-users", type=int, default=2048)
    print(json.dumps(bench(ap.parse_args())), flush=True)


if __name__ == "__main__":
    main()
