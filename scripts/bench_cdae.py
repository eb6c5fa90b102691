"""Step time and score() throughput of the CDAE engine (neurec_amd/cdae.py) at the reference's defaults on gowalla's
counts, beside a torch-autograd statement of the same step on the same device.

    python scripts/bench_cdae.py [--steps 200] [--warmup 30] [--repeats 5] [--torch-steps 100] [--score-users 2048]
                                 [--out profiles/r25_cdae.json] [--trace [--trace-out profiles/r25_cdae_trace.json]]

conf/CDAE.properties: hidden_dim 64, batch 32 users, num_neg 5, dropout 0.5, sigmoid, sigmoid_cross_entropy, reg 0.001,
Adam at 0.001.  U = 29,858, I = 40,981, 813,886 train entries (neurec_amd/synth.py).  In ONE process, `--repeats`
windows of `--steps` engine steps and of `--torch-steps` steps of the torch statement, INTERLEAVED, each timed between
device events after a warm-up: the median window and the range, in ms per step.

    engine      ms_per_step: batch building, the gradient call and the five applications; batch_ms / grad_ms / apply_ms:
                each alone (launch-bound loops, not a split); with --trace the device time per kernel from the
                profiler's trace of 20 steps, in a run of its own
    torch       the same step on batches the engine built (the torch side builds none): index_add pooling, gathers, the
                loss, the regulariser on the unique items, autograd, torch.optim.Adam — dense on every variable, as
                the engine's sparse Adam sweeps every row
    bound       the bytes the Adam sweep of the four row tables must move once (4 reads + 3 writes per float) over the
                measured HBM copy rate
    score       users / s of score() (the encoder on train rows, then the fp32-MFMA GEMM against [de | bias]) and the
                time of a full evaluation's scores at that rate

One JSON line, written to --out as well.
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

HBM_RATE = 6.29e12
D, BATCH, NUM_NEG, DROPOUT, REG, LR = 64, 32, 5, 0.5, 0.001, 0.001


def _torch_step_fn(tables, keep_prob):
    """fn(batch, keep) on the engine's device batch: the graph of CDAE.py:62-98 with torch ops, then Adam"""
    import torch
    P = {k: torch.from_numpy(v).to("cuda").requires_grad_() for k, v in tables.items()}
    opt = torch.optim.Adam(list(P.values()), lr=LR, betas=(0.9, 0.999), eps=1e-8)
    bce = torch.nn.functional.binary_cross_entropy_with_logits

    def step(b, keep):
        users, items, slot, in_items, in_slot, labels = b
        val = keep.float() * (1.0 / keep_prob)
        pooled = torch.zeros((users.numel(), D), device="cuda").index_add(0, in_slot,
                                                                          P["en_embeddings"][in_items] * val[:, None])
        hidden = torch.sigmoid(pooled + P["user_embeddings"][users] + P["en_offset"])
        x = (hidden[slot] * P["de_embeddings"][items]).sum(1) + P["de_bias"][items]
        uniq = torch.unique(items)
        l2 = sum((t * t).sum() for t in (P["en_embeddings"][uniq], P["de_embeddings"][uniq], P["de_bias"][uniq],
                                         P["user_embeddings"][users], P["en_offset"])) / 2
        loss = bce(x, labels, reduction="sum") + REG * l2
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss
    return step


def _kernel_trace(step, n=20):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for k in range(n):
                step(k)
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
            if t and any(s in ev.key for s in ("cdae", "sort", "adam", "Memcpy", "score_gemm")):
                out[ev.key[:80]] = t / n
        return out or None
    except Exception as exc:                                    # the figures above do not depend on it
        return {"error": repr(exc)[:200]}


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=100)
    ap.add_argument("--score-users", type=int, default=2048)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_cdae.json"))
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "r25_cdae_trace.json"))
    a = ap.parse_args()
    from neurec_amd import engine as E, synth
    from neurec_amd.cdae import CDAEEngine
    from neurec_amd.model.general_recommender.CDAE import initial_variables
    train, _ = synth.interactions("gowalla")
    U, I = train.shape
    tables = initial_variables(U, I, D)
    eng = CDAEEngine(tables, train, LR, REG, DROPOUT, NUM_NEG, BATCH)
    dev = eng.T["en_offset"].device
    rs = np.random.RandomState(0)
    active = np.flatnonzero(np.diff(train.indptr) > 0)
    n_feed = 32
    feeds = [rs.choice(active, BATCH, replace=False).astype(np.int32) for _ in range(n_feed)]
    loss2 = torch.zeros(2, device=dev)
    step = lambda k: eng.step(feeds[k % n_feed], loss2)
    _timed(step, a.warmup)
    if a.trace:                                                  # a run of its own: the profiler slows the windows
        line = json.dumps({"kernel_us_per_step": _kernel_trace(step)})
        print(line)
        if a.trace_out:
            os.makedirs(os.path.dirname(a.trace_out), exist_ok=True)
            with open(a.trace_out, "w") as f:
                f.write(line + "\n")
        return
    batches = [eng.batch(f, eng.step_seed()) for f in feeds]
    entries = float(np.mean([int(b.entry_ptr[-1].item()) for b in batches]))
    tstep = None
    if a.torch_steps:
        fn = _torch_step_fn(tables, eng.keep_prob)
        tb = []
        for b in batches:
            n = int(b.entry_ptr[-1].item())
            in_slot = torch.repeat_interleave(torch.arange(b.B, device=dev), b.entry_ptr[1:] - b.entry_ptr[:-1])
            tb.append(((b.users.long(), b.items[:n].long(), b.slot[:n].long(), b.in_items[:n].long(), in_slot,
                        b.labels[:n]), torch.rand(n, device=dev) < eng.keep_prob))
        tstep = lambda k: fn(*tb[k % n_feed])
        _timed(tstep, max(a.warmup // 3, 5))
    windows, tw = [], []
    for _ in range(a.repeats):                                   # interleaved: both see the same state of the machine
        windows.append(_timed(step, a.steps))
        if tstep is not None:
            tw.append(_timed(tstep, a.torch_steps))
    windows.sort()
    tw.sort()
    batch_ms = _timed(lambda k: eng.batch(feeds[k % n_feed], k), a.steps)
    grad_ms = _timed(lambda k: eng.gradients(batches[k % n_feed], loss2), a.steps)
    for g in eng.G.values():
        g.zero_()
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    # batch: draw, sort, count, fill; step: keys, forward, sort, rows, loss; sparse Adam x 4, ApplyAdam x 1
    launches = {"nrhip_cdae_batch": 4, "nrhip_cdae_step": 5, "apply": 5, "h2d_copies": 2}
    out = {"device": E.device_info() if hasattr(E, "device_info") else None,
           "shape": {"n_users": U, "n_items": I, "nnz": int(train.nnz), "hidden_dim": D, "batch_users": BATCH,
                     "num_neg": NUM_NEG, "entries_per_step": entries},
           "engine": {"ms_per_step": windows[len(windows) // 2], "min": windows[0], "max": windows[-1],
                      "batch_ms": batch_ms, "grad_ms": grad_ms, "apply_ms": apply_ms, "launches": launches}}
    if tw:
        out["torch"] = {"ms_per_step": tw[len(tw) // 2], "min": tw[0], "max": tw[-1]}
        out["engine_over_torch"] = out["engine"]["ms_per_step"] / out["torch"]["ms_per_step"]
    nbytes = 7 * 4 * ((U + 2 * I) * D + I + D)
    out["bound"] = {"bytes": nbytes, "hbm_ms": nbytes / HBM_RATE * 1e3}
    out["step_over_bound"] = out["engine"]["ms_per_step"] / out["bound"]["hbm_ms"]
    out["apply_over_bound"] = apply_ms / out["bound"]["hbm_ms"]

    n = a.score_users
    su = rs.randint(0, U, n).astype(np.int32)
    score = lambda k: eng.score(su)
    _timed(score, 3)
    sm = sorted(_timed(score, 5) for _ in range(5))
    ms = sm[len(sm) // 2]
    flop = 2.0 * n * I * (D + 1)
    out["score"] = {"users": n, "ms": ms, "min": sm[0], "max": sm[-1], "users_per_s": n / ms * 1e3,
                    "tflops": flop / ms / 1e9, "full_eval_ms": U / (n / ms),
                    "write_floor_ms": 4.0 * n * I / HBM_RATE * 1e3}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
