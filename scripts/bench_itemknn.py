"""Build time and scoring rate of the ItemKNN engine (neurec_amd/itemknn.py) on the gowalla and ml-100k shapes.

    python scripts/bench_itemknn.py [--shapes gowalla,ml-100k] [--neighbors 5,100] [--similarity cosine]
                                    [--batch 1024] [--repeats 5]

Per (shape, neighbor): `build_ms`, the wall time of one ItemKNNEngine construction after a warm-up one (the host's
O(nnz) float64 preparation and the upload included), and `users_per_s`, from `--repeats` score calls of `--batch` users each timed between device events (median).
The algorithmic work it is set against:

    build   co-occurrence walk sum_u deg(u)^2 multiply-adds; the elementwise pass, the selection's radix passes and the
            gather read the I-long accumulator column about 7 times per column: ~ 7 I^2 4 bytes of LDS or L2 traffic
    score   sum over the batch of sum_{j in N(u)} len(W row j) multiply-adds, 8 bytes read (index, value) and a 4-byte
            read-modify-write of the score row each, plus the row's zero fill I 4 bytes

One JSON line per (shape, neighbor).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def bench(shape, neighbor, similarity, batch, repeats):
    import numpy as np
    import torch
    from neurec_amd import itemknn, synth
    train, _ = synth.interactions(shape)
    U, I = train.shape
    itemknn.ItemKNNEngine(train, neighbor, 0, similarity)          # warm-up: module load, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng = itemknn.ItemKNNEngine(train, neighbor, 0, similarity)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    rng = np.random.RandomState(7)
    users = torch.from_numpy(rng.randint(0, U, batch).astype(np.int32)).cuda()
    out = torch.empty((batch, I), dtype=torch.float32, device="cuda")
    eng.score(users, out=out)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(repeats + 1)]
    ev[0].record()
    for r in range(repeats):
        eng.score(users, out=out)
        ev[r + 1].record()
    torch.cuda.synchronize()
    score_ms = sorted(ev[r].elapsed_time(ev[r + 1]) for r in range(repeats))[repeats // 2]
    assert bool(torch.isfinite(out).all())
    deg = np.diff(train.tocsr().indptr).astype(np.float64)
    row_len = np.diff(eng.t_indptr.cpu().numpy())
    csr = train.tocsr()
    terms = float(sum(row_len[csr.indices[csr.indptr[u]:csr.indptr[u + 1]]].sum() for u in users.cpu().numpy()))
    return {"shape": shape, "users": U, "items": I, "nnz": int(train.nnz), "similarity": similarity,
            "neighbor": neighbor, "column_in_lds": bool(I <= itemknn.LDS_ITEMS), "block_cols": eng.block_cols,
            "w_nnz": int(row_len.sum()), "longest_w_row": int(row_len.max()), "build_ms": round(build_ms, 3),
            "cooccurrence_madds": float((deg ** 2).sum()), "batch": batch, "score_ms": round(score_ms, 4),
            "users_per_s": round(batch / (score_ms * 1e-3), 1), "score_madds_per_batch": terms,
            "score_gmadds_per_s": round(terms / (score_ms * 1e-3) / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="gowalla,ml-100k")
    ap.add_argument("--neighbors", default="5,100")
    ap.add_argument("--similarity", default="cosine")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        for k in (int(x) for x in a.neighbors.split(",")):
            print(json.dumps(bench(shape, k, a.similarity, a.batch, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
