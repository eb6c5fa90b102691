"""Epoch time of the WRMF engine (neurec_amd/wrmf.py) on the gowalla and ml-100k shapes, with its share of peak.

    python scripts/bench_wrmf.py [--epochs 5] [--shapes gowalla,ml-100k] [--dims 16,64]

One warm-up epoch, then `--epochs` epochs timed between device events: ms per epoch and per half-sweep (users,
items).  The algorithmic work of a half that solves R rows against a table of n rows, nnz neighbour entries:

    FLOP   Gram 2 n d^2  +  accumulation 2 nnz d^2  +  factorisation R d^3 / 3  +  solves 2 R d^2
    bytes  gathered neighbour rows nnz d 4

and the share of peak is the larger of FLOP / 157 TF (fp32 matrix peak) and bytes / 8 TB/s (HBM), over the time.
One JSON line per (shape, d).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FLOPS = 157e12      # fp32 matrix (MI355X_MICROARCH.md)
PEAK_BYTES = 8e12        # HBM3E


def half_work(n_other, n_rows, nnz, d):
    flop = 2.0 * n_other * d * d + 2.0 * nnz * d * d + n_rows * d ** 3 / 3.0 + 2.0 * n_rows * d * d
    return flop, 4.0 * nnz * d


def bench(shape, d, epochs):
    import numpy as np
    import torch
    from neurec_amd import synth
    from neurec_amd.wrmf import WRMFEngine
    train, _ = synth.interactions(shape)
    U, I = train.shape
    rng = np.random.RandomState(2017)
    eng = WRMFEngine(rng.uniform(-0.01, 0.01, (U, d)), rng.uniform(-0.01, 0.01, (I, d)), train, 10.0, 0.1)
    eng.epoch()                                   # warm-up
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * epochs + 1)]
    ev[0].record()
    for e in range(epochs):
        eng.solve_users()
        ev[2 * e + 1].record()
        eng.solve_items()
        ev[2 * e + 2].record()
    torch.cuda.synchronize()
    users_ms = sorted(ev[2 * e].elapsed_time(ev[2 * e + 1]) for e in range(epochs))[epochs // 2]
    items_ms = sorted(ev[2 * e + 1].elapsed_time(ev[2 * e + 2]) for e in range(epochs))[epochs // 2]
    epoch_ms = ev[0].elapsed_time(ev[-1]) / epochs
    nnz = train.nnz
    fu, bu = half_work(I, U, nnz, d)
    fi, bi = half_work(U, I, nnz, d)
    P, Q = eng.tables()
    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(Q).all())
    share = max((fu + fi) / PEAK_FLOPS, (bu + bi) / PEAK_BYTES) / (epoch_ms * 1e-3)
    return {"shape": shape, "users": U, "items": I, "nnz": nnz, "d": d, "epochs_timed": epochs,
            "epoch_ms": round(epoch_ms, 4), "users_half_ms": round(users_ms, 4), "items_half_ms": round(items_ms, 4),
            "chunks_users": eng.users.n_chunks, "chunks_items": eng.items.n_chunks,
            "gflop_per_epoch": round((fu + fi) / 1e9, 3), "gathered_mb_per_epoch": round((bu + bi) / 1e6, 2),
            "tflops": round((fu + fi) / (epoch_ms * 1e-3) / 1e12, 3), "share_of_peak": round(share, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--shapes", default="gowalla,ml-100k")
    ap.add_argument("--dims", default="16,64")
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        for d in (int(x) for x in a.dims.split(",")):
            print(json.dumps(bench(shape, d, a.epochs)), flush=True)


if __name__ == "__main__":
    main()
