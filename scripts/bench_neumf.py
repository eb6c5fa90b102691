"""Step time and score() throughput of the NeuMF engine (neurec_amd/neumf.py) at the reference's defaults on gowalla's
user and item counts, beside torch-on-device statements of the same step and of the same scores.

    python scripts/bench_neumf.py [--steps 200] [--warmup 30] [--repeats 5] [--batch 256] [--torch-steps 100]
                                  [--score-users 2048] [--torch-score-users 64] [--trace]

conf/NeuMF.properties: embedding_size 16, layers [64,32,16], batch 256, cross_entropy, adam, lr 0.001, no regulariser.
U = 29,858, I = 40,981.  The instances are synthetic: users and items uniform over their tables, one label in five 1 —
the step's cost does not depend on which ids they are.  In ONE process, `--repeats` windows of `--steps` steps of the
engine and of `--torch-steps` steps of the torch statement, INTERLEAVED, each timed between device events after a
warm-up: the median window and the range, in ms per step.

    engine          ms_per_step (median, min, max), grad_ms / apply_ms (nrhip_neumf_step alone and the learner's
                    applications alone: launch-bound loops, not a split), launches per step; with --trace the device
                    time per kernel name from the profiler's trace of 20 steps
    torch           the same step written with torch ops on the device (gathers, matmuls, relu, the loss, autograd,
                    torch.optim.Adam — dense on every variable, so the sweeps of the four tables are in it as they are
                    in the engine's sparse Adam)
    score           users / s of score() and TFLOP/s on the per-pair count 2 sum_{k >= 2} in_k out_k plus the adds (the
                    first activation's layers[0], the row sum's layers[-1], the GMF dot's 2 d), against the 155 TF
                    fp32-MFMA ceiling; full_eval_ms: all U users at that rate; floor_ms: the count over the ceiling
    torch_score     the same for the torch statement, which materialises [n I, layers[0]]
    bound           the step's multiply-adds (forward and twice that backward) over the fp32 VALU rate, and the bytes it
                    must move once (sparse Adam's sweep of the four tables: 4 reads + 3 writes) over the measured HBM
                    copy rate; bound_ms is the larger

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
HBM_RATE = 6.29e12
N_USERS, N_ITEMS = 29858, 40981
D, LAYERS, LR = 16, [64, 32, 16], 0.001
E_HALF = LAYERS[0] // 2
INS = [2 * E_HALF] + LAYERS[:-1]


def _tables():
    from neurec_amd.model.general_recommender.NeuMF import initial_variables
    return initial_variables(N_USERS, N_ITEMS, D, LAYERS, "normal", 0.01)


def _feeds(steps, batch, seed=0):
    import numpy as np
    rs = np.random.RandomState(seed)
    return rs.randint(0, N_USERS, (steps, batch)).astype(np.int32), \
        rs.randint(0, N_ITEMS, (steps, batch)).astype(np.int32), (rs.rand(steps, batch) < 0.2).astype(np.float32)


def _torch_forward(P, users, items):
    import torch
    h = torch.cat([P["mlp_embedding_user"][users], P["mlp_embedding_item"][items]], dim=1)
    for k in range(len(LAYERS)):
        h = torch.relu(h @ P["kernel%d" % k] + P["bias%d" % k])
    return h.sum(1) + (P["mf_embedding_user"][users] * P["mf_embedding_item"][items]).sum(1)


def _torch_step_fn(tables):
    """the step as torch ops + autograd + torch.optim.Adam; returns fn(users, items, labels) on device tensors"""
    import torch
    P = {k: torch.from_numpy(v).to("cuda").requires_grad_() for k, v in tables.items()}
    opt = torch.optim.Adam(list(P.values()), lr=LR, betas=(0.9, 0.999), eps=1e-8)
    bce = torch.nn.functional.binary_cross_entropy_with_logits

    def step(users, items, labels):
        loss = bce(_torch_forward(P, users, items), labels)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss
    return step


def _torch_score_fn(tables):
    """[n, I] scores with torch ops: every (user, item) pair's concat row is materialised, [n I, layers[0]]"""
    import torch
    P = {k: torch.from_numpy(v).to("cuda") for k, v in tables.items()}
    all_items = torch.arange(N_ITEMS, device="cuda")

    def score(users):
        n = users.numel()
        with torch.no_grad():
            return _torch_forward(P, users.repeat_interleave(N_ITEMS), all_items.repeat(n)).view(n, N_ITEMS)
    return score


def _kernel_trace(step, n=20):
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
            if t and ("neumf" in ev.key or "sort" in ev.key or "adam" in ev.key or "optimizer" in ev.key):
                out[ev.key[:80]] = t / n
        return out or None
    except Exception as exc:                                    # the figures above do not depend on it
        return {"error": repr(exc)[:200]}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--torch-steps", type=int, default=100)
    ap.add_argument("--score-users", type=int, default=2048)
    ap.add_argument("--torch-score-users", type=int, default=64)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    from neurec_amd import engine as E
    from neurec_amd.neumf import NeuMFEngine
    tables = _tables()
    eng = NeuMFEngine(tables, LAYERS, LR, 0.0, 0.0, a.batch)
    dev = eng.T["mlp_embedding_user"].device
    n_feed = 32
    users, items, labels = (torch.from_numpy(x).to(dev) for x in _feeds(n_feed, a.batch))
    loss2 = torch.zeros(2, device=dev)

    def step(k):
        j = k % n_feed
        eng.step(users[j], items[j], labels[j], loss2)
    _timed(step, a.warmup)
    tstep = None
    if a.torch_steps:
        fn = _torch_step_fn(tables)
        u64, i64 = users.long(), items.long()
        tstep = lambda k: fn(u64[k % n_feed], i64[k % n_feed], labels[k % n_feed])
        _timed(tstep, max(a.warmup // 3, 5))
    windows, tw = [], []
    for _ in range(a.repeats):                                   # interleaved: both see the same state of the machine
        windows.append(_timed(step, a.steps))
        if tstep is not None:
            tw.append(_timed(tstep, a.torch_steps))
    windows.sort()
    tw.sort()
    grad_ms = _timed(lambda k: eng.gradients(users[k % n_feed], items[k % n_feed], labels[k % n_feed], loss2), a.steps)
    for g in eng.G.values():
        g.zero_()
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    # row, reduce, sort, rows, loss; sparse Adam x 4 tables, dense Adam on the 6 variables in one launch
    launches = {"nrhip_neumf_step": 5, "apply": 4 + 1}
    out = {"device": E.device_info() if hasattr(E, "device_info") else None,
           "shape": {"n_users": N_USERS, "n_items": N_ITEMS, "embedding_size": D, "layers": LAYERS, "batch": a.batch},
           "engine": {"ms_per_step": windows[len(windows) // 2], "min": windows[0], "max": windows[-1],
                      "grad_ms": grad_ms, "apply_ms": apply_ms, "launches_per_step": sum(launches.values()),
                      "launches": launches}}
    if a.trace:
        out["engine"]["kernel_us_per_step"] = _kernel_trace(step)
    if tw:
        out["torch"] = {"ms_per_step": tw[len(tw) // 2], "min": tw[0], "max": tw[-1]}
        out["engine_over_torch"] = out["engine"]["ms_per_step"] / out["torch"]["ms_per_step"]
    fwd = sum(i * w for i, w in zip(INS, LAYERS)) + D
    macs = a.batch * 3 * fwd
    table_floats = (N_USERS + N_ITEMS) * (D + E_HALF)
    nbytes = 7 * table_floats * 4
    out["bound"] = {"multiply_adds": macs, "valu_ms": macs / VALU_RATE * 1e3, "bytes": nbytes,
                    "hbm_ms": nbytes / HBM_RATE * 1e3}
    out["bound"]["bound_ms"] = max(out["bound"]["valu_ms"], out["bound"]["hbm_ms"])
    out["step_over_bound"] = out["engine"]["ms_per_step"] / out["bound"]["bound_ms"]

    # ---- score(): every item for n users
    flop_per_pair = 2 * sum(i * w for i, w in zip(INS[1:], LAYERS[1:])) + LAYERS[0] + LAYERS[-1] + 2 * D
    floor_ms = N_USERS * N_ITEMS * flop_per_pair / MFMA_F32_RATE * 1e3
    n = a.score_users
    su = torch.from_numpy(_feeds(1, n, seed=1)[0][0]).to(dev)
    buf = torch.empty((n, N_ITEMS), dtype=torch.float32, device=dev)
    score = lambda k: eng.score(su, out=buf)
    _timed(score, 3)
    sm = sorted(_timed(score, 5) for _ in range(5))
    ms = sm[len(sm) // 2]
    out["score"] = {"users": n, "ms": ms, "min": sm[0], "max": sm[-1], "users_per_s": n / ms * 1e3,
                    "flop_per_pair": flop_per_pair, "tflops": n * N_ITEMS * flop_per_pair / ms / 1e9,
                    "of_ceiling": n * N_ITEMS * flop_per_pair / ms / 1e9 / (MFMA_F32_RATE / 1e12),
                    "full_eval_ms": N_USERS / (n / ms), "floor_ms": floor_ms}
    out["score"]["full_eval_over_floor"] = out["score"]["full_eval_ms"] / floor_ms
    if a.torch_score_users:
        nt = a.torch_score_users
        tscore_fn = _torch_score_fn({k: t.cpu().numpy() for k, t in eng.tables().items()})    # as the steps left them
        tu = su[:nt].long()
        tscore = lambda k: tscore_fn(tu)
        _timed(tscore, 2)
        tm = sorted(_timed(tscore, 3) for _ in range(3))[1]
        out["torch_score"] = {"users": nt, "ms": tm, "users_per_s": nt / tm * 1e3,
                              "tflops": nt * N_ITEMS * flop_per_pair / tm / 1e9,
                              "full_eval_ms": N_USERS / (nt / tm)}
        out["score_over_torch"] = out["score"]["users_per_s"] / out["torch_score"]["users_per_s"]
        got, want = eng.score(tu.int())[:nt], tscore_fn(tu)
        out["score_vs_torch"] = {"max_err": float((got - want).abs().max()), "max_abs": float(want.abs().max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
