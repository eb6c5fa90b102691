"""Step time and score() throughput of the ConvNCF engine (neurec_amd/convncf.py) at the reference's defaults on gowalla's
user and item counts, beside torch-on-device statements of the same step and of the same scores.

    python scripts/bench_convncf.py [--steps 20] [--warmup 5] [--repeats 5] [--batch 512] [--torch-steps 10]
                                    [--score-users 16] [--torch-score-users 2] [--trace]

conf/ConvNCF.properties: embedding_size 64, net_channel [32] * 6, batch 512, BPR, regs [0.01, 0, 0], lr_embed = lr_net =
0.05.  U = 29,858, I = 40,981.  The triplets are synthetic: users and items uniform over their tables — the step's cost
does not depend on which ids they are.  In ONE process, `--repeats` windows of `--steps` steps of the engine and of
`--torch-steps` steps of the torch statement, INTERLEAVED, each timed between device events after a warm-up: the median
window and the range, in ms per step.

    engine          ms_per_step (median, min, max), grad_ms / apply_ms (nrhip_convncf_step alone and the two Adagrad
                    applications alone); with --trace the device time per kernel name from the profiler's trace
    torch           the same step written with torch ops on the device (gathers, the outer product, F.conv2d at stride 2,
                    tanh, the loss, autograd, torch.optim.Adagrad from 0.1 — dense on every variable)
    score           users / s of score() over `--score-users` users x all items, TFLOP/s on the 3.06 Mflop per pair of the
                    multiply-adds, against the 155 TF fp32-MFMA ceiling; never a whole evaluation (1.22 G pairs)
    torch_score     the same for the torch statement, in chunks of items that fit its activations
    bound           the step's multiply-adds (forward and twice that backward) over the fp32 VALU rate — the kernels here
                    run on the vector unit — and over the fp32-MFMA ceiling

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

from bench_fpmc import _timed          # noqa: E402

VALU_RATE = 157.3e12 / 4
MFMA_F32_RATE = 155e12
N_USERS, N_ITEMS = 29858, 40981
D, CHANNELS, LR, REGS = 64, [32] * 6, 0.05, [0.01, 0.0, 0.0]


def macs_per_pair():
    """multiply-adds of one inference: layer k has (D >> k)^2 positions of 4 c_in c_out, then the head"""
    c_in, total = 1, 0
    for k, c in enumerate(CHANNELS, 1):
        total += (D >> k) ** 2 * 4 * c_in * c
        c_in = c
    return total + c_in


def _tables():
    from neurec_amd.model.general_recommender.ConvNCF import initial_variables
    return initial_variables(N_USERS, N_ITEMS, D, CHANNELS, "tnormal", "xavier_normal", 0.01)


def _feeds(steps, batch, seed=0):
    import numpy as np
    rs = np.random.RandomState(seed)
    return tuple(rs.randint(0, n, (steps, batch)).astype(np.int32) for n in (N_USERS, N_ITEMS, N_ITEMS))


def _torch_forward(P, users, items):
    import torch
    import torch.nn.functional as F
    x = (P["embedding_P"][users][:, :, None] * P["embedding_Q"][items][:, None, :])[:, None]
    for k in range(len(CHANNELS)):
        x = torch.tanh(F.conv2d(x, P["kernel%d" % k].permute(3, 2, 0, 1), P["bias%d" % k], stride=2))
    return x.reshape(x.shape[0], -1) @ P["W"][:, 0] + P["b"][0]


def _torch_step_fn(tables):
    """the step as torch ops + autograd + torch.optim.Adagrad; returns fn(users, pos, neg) on device tensors"""
    import torch
    P = {k: torch.from_numpy(v).to("cuda").requires_grad_() for k, v in tables.items()}
    opt = torch.optim.Adagrad(list(P.values()), lr=LR, initial_accumulator_value=0.1, eps=0.0)

    def step(users, pos, neg):
        y = _torch_forward(P, users, pos) - _torch_forward(P, users, neg)
        p, q1, q2 = P["embedding_P"][users], P["embedding_Q"][pos], P["embedding_Q"][neg]
        loss = -torch.nn.functional.logsigmoid(y).sum() + REGS[0] * 0.5 * ((p * p).sum() + (q1 * q1).sum() + (q2 * q2).sum())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss
    return step


def _torch_score_fn(tables, chunk=2048):
    """[n, I] scores with torch ops, `chunk` items at a time: layer 1 alone is 128 KB per pair"""
    import torch
    P = {k: torch.from_numpy(v).to("cuda") for k, v in tables.items()}

    def score(users):
        out = torch.empty((users.numel(), N_ITEMS), device="cuda")
        with torch.no_grad():
            for r, u in enumerate(users):
                for i0 in range(0, N_ITEMS, chunk):
                    items = torch.arange(i0, min(i0 + chunk, N_ITEMS), device="cuda")
                    out[r, i0:i0 + len(items)] = _torch_forward(P, u.expand(len(items)), items)
        return out
    return score


def _kernel_trace(step, n=5):
    """{kernel name: device us per step} from the profiler's trace of n steps; None where it is not available"""
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
            if t and ("convncf" in ev.key or "sort" in ev.key or "optimizer" in ev.key):
                out[ev.key[:80]] = t / n
        return out or None
    except Exception as exc:                                    # the figures above do not depend on it
        return {"error": repr(exc)[:200]}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--torch-steps", type=int, default=10)
    ap.add_argument("--score-users", type=int, default=16)
    ap.add_argument("--torch-score-users", type=int, default=2)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if a.score_users > 64:
        raise SystemExit("--score-users is at most 64: a block of users, never a whole evaluation")
    from neurec_amd import engine as E
    from neurec_amd.convncf import ConvNCFEngine
    tables = _tables()
    eng = ConvNCFEngine(tables, CHANNELS, LR, LR, REGS, a.batch)
    dev = eng.T["embedding_P"].device
    n_feed = 8
    users, pos, neg = (torch.from_numpy(x).to(dev) for x in _feeds(n_feed, a.batch))
    loss2 = torch.zeros(2, device=dev)

    def step(k):
        j = k % n_feed
        eng.step(users[j], pos[j], neg[j], loss2)
    _timed(step, a.warmup)
    tstep = None
    if a.torch_steps:
        fn = _torch_step_fn(tables)
        u64, p64, n64 = users.long(), pos.long(), neg.long()
        tstep = lambda k: fn(u64[k % n_feed], p64[k % n_feed], n64[k % n_feed])
        _timed(tstep, max(a.warmup // 2, 2))
    windows, tw = [], []
    for _ in range(a.repeats):                                   # interleaved: both see the same state of the machine
        windows.append(_timed(step, a.steps))
        if tstep is not None:
            tw.append(_timed(tstep, a.torch_steps))
    windows.sort()
    tw.sort()
    grad_ms = _timed(lambda k: eng.gradients(users[k % n_feed], pos[k % n_feed], neg[k % n_feed], loss2), a.steps)
    for g in eng.G.values():
        g.zero_()
    for f in eng.flag.values():
        f.zero_()
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    out = {"device": E.device_info() if hasattr(E, "device_info") else None,
           "shape": {"n_users": N_USERS, "n_items": N_ITEMS, "embedding_size": D, "net_channel": CHANNELS,
                     "batch": a.batch},
           "engine": {"ms_per_step": windows[len(windows) // 2], "min": windows[0], "max": windows[-1],
                      "grad_ms": grad_ms, "apply_ms": apply_ms, "workspace_mb": eng.workspace_floats() * 4 / 2 ** 20}}
    if a.trace:
        out["engine"]["kernel_us_per_step"] = _kernel_trace(step)
    if tw:
        out["torch"] = {"ms_per_step": tw[len(tw) // 2], "min": tw[0], "max": tw[-1]}
        out["engine_over_torch"] = out["engine"]["ms_per_step"] / out["torch"]["ms_per_step"]
    fwd = macs_per_pair()
    macs = 2 * a.batch * (3 * fwd + (D // 2) ** 2 * 4 * CHANNELS[0])      # three passes, and layer 1 is made twice
    out["bound"] = {"multiply_adds_per_pair": fwd, "tanh_per_pair": sum((D >> k) ** 2 * c for k, c in
                                                                         enumerate(CHANNELS, 1)),
                    "multiply_adds": macs, "valu_ms": macs / VALU_RATE * 1e3, "mfma_ms": 2 * macs / MFMA_F32_RATE * 1e3}
    out["step_over_valu_bound"] = out["engine"]["ms_per_step"] / out["bound"]["valu_ms"]

    # ---- score(): every item for a block of users
    flop_per_pair = 2 * fwd
    n = a.score_users
    su = torch.from_numpy(_feeds(1, n, seed=1)[0][0]).to(dev)
    buf = torch.empty((n, N_ITEMS), dtype=torch.float32, device=dev)
    score = lambda k: eng.score(su, out=buf)
    _timed(score, 1)
    sm = sorted(_timed(score, 2) for _ in range(5))
    ms = sm[len(sm) // 2]
    out["score"] = {"users": n, "ms": ms, "min": sm[0], "max": sm[-1], "users_per_s": n / ms * 1e3,
                    "flop_per_pair": flop_per_pair, "tflops": n * N_ITEMS * flop_per_pair / ms / 1e9,
                    "of_ceiling": n * N_ITEMS * flop_per_pair / ms / 1e9 / (MFMA_F32_RATE / 1e12),
                    "of_valu_rate": n * N_ITEMS * flop_per_pair / ms / 1e9 / (2 * VALU_RATE / 1e12)}
    if a.torch_score_users:
        nt = min(a.torch_score_users, n)
        tscore_fn = _torch_score_fn({k: t.cpu().numpy() for k, t in eng.tables().items()})    # as the steps left them
        tu = su[:nt].long()
        tscore = lambda k: tscore_fn(tu)
        _timed(tscore, 1)
        tm = sorted(_timed(tscore, 1) for _ in range(3))[1]
        out["torch_score"] = {"users": nt, "ms": tm, "users_per_s": nt / tm * 1e3,
                              "tflops": nt * N_ITEMS * flop_per_pair / tm / 1e9}
        out["score_over_torch"] = out["score"]["users_per_s"] / out["torch_score"]["users_per_s"]
        got, want = eng.score(tu.int())[:nt], tscore_fn(tu)
        out["score_vs_torch"] = {"max_err": float((got - want).abs().max()), "max_abs": float(want.abs().max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
