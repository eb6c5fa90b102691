"""The APR step (neurec_amd/apr.py, csrc/apr.hip) on the gowalla shape.

    python scripts/bench_apr.py [--shape gowalla] [--steps 200] [--warmup 20] [--batch 512] [--d 64] [--out FILE]

The train matrix is the synthetic gowalla-shaped one of neurec_amd/synth.py; the hyper-parameters are
conf/APR.properties' (d = 64, B = 512, adam, adv = grad, reg = 0, reg_adv = 1, eps = 0.5).  The batches are uniform
train pairs with a uniform negative each.  Five windows of `--steps` steps between device events are taken per figure,
the contenders interleaved window by window, and the median is reported (`*_windows`: all five):

    adversarial   APREngine.step(adversarial=True): both passes and the two Adam sweeps
    plain         APREngine.step(adversarial=False): one pass and the sweeps
    torch         an eager torch autograd statement of the same two-pass step (gradient of the plain loss, normalised
                  Delta detached, opt_loss, backward, torch.optim.Adam) on the same device
    mf            GeneralMFEngine's BPR / adam step: what one pass costs here — APR gathers every row twice and runs
                  two rows passes
    grad / apply  nrhip_apr_step alone (adversarial and plain) and the two applications alone

`apply_bound_ms` is the Adam sweep's traffic at 8 TB/s: the variable and both moments read and written and the
gradient read and cleared, 8 floats per entry of (U + I) d.  One JSON line.
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

HBM_BYTES_PER_S = 8.0e12
LR, REG_ADV, EPS, WINDOWS = 0.001, 1.0, 0.5, 5


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def torch_step_fn(P0, Q0):
    import torch
    import torch.nn.functional as F
    P = torch.from_numpy(P0).cuda().requires_grad_(True)
    Q = torch.from_numpy(Q0).cuda().requires_grad_(True)
    opt = torch.optim.Adam([P, Q], lr=LR)

    def loss_of(p, qi, qj):
        return F.softplus(-((p * qi).sum(1) - (p * qj).sum(1))).sum()

    def norm(g):
        return (g * torch.rsqrt(torch.clamp((g * g).sum(1, keepdim=True), min=1e-12)) * EPS).detach()

    def step(u, i, j):
        p, qi, qj = P[u], Q[i], Q[j]
        loss = loss_of(p, qi, qj)
        gp, gqi, gqj = torch.autograd.grad(loss, [p, qi, qj], retain_graph=True)
        # Delta of a row = the normalised SUM of its occurrences' gradients: scatter, normalise, gather
        GP = torch.zeros_like(P).index_add_(0, u, gp)
        GQ = torch.zeros_like(Q).index_add_(0, i, gqi).index_add_(0, j, gqj)
        DP, DQ = norm(GP), norm(GQ)
        total = loss + REG_ADV * loss_of(p + DP[u], qi + DQ[i], qj + DQ[j])
        opt.zero_grad(set_to_none=False)
        total.backward()
        opt.step()
    return step


def bench(a):
    import numpy as np
    import torch
    from neurec_amd import synth
    from neurec_amd.apr import APREngine
    from neurec_amd.trainer import GeneralMFEngine
    train, _ = synth.interactions(a.shape)
    train = train.tocoo()
    U, I = train.shape
    d, B, need = a.d, a.batch, a.warmup + a.steps
    rs = np.random.RandomState(7)
    P0, Q0 = (0.01 * rs.randn(U, d)).astype(np.float32), (0.01 * rs.randn(I, d)).astype(np.float32)
    pick = rs.randint(0, train.nnz, (need, B))
    users = torch.from_numpy(train.row[pick].astype(np.int32)).cuda()
    pos = torch.from_numpy(train.col[pick].astype(np.int32)).cuda()
    neg = torch.from_numpy(rs.randint(0, I, (need, B)).astype(np.int32)).cuda()
    users64, pos64, neg64 = users.long(), pos.long(), neg.long()
    eng = APREngine(P0, Q0, LR, 0.0, REG_ADV, EPS, B)
    mf = GeneralMFEngine(P0, Q0, LR, 0.0, B)
    tstep = torch_step_fn(P0, Q0)
    losses = torch.zeros((need, 2), device="cuda")
    runs = {
        "adversarial": lambda k: eng.step(users[k], pos[k], neg[k], losses[k], adversarial=True),
        "plain": lambda k: eng.step(users[k], pos[k], neg[k], losses[k], adversarial=False),
        "torch": lambda k: tstep(users64[k], pos64[k], neg64[k]),
        "mf": lambda k: mf.step(users[k], pos[k], neg[k], losses[k]),
        "grad_adversarial": lambda k: eng.gradients(users[k], pos[k], neg[k], losses[k], adversarial=True),
        "grad_plain": lambda k: eng.gradients(users[k], pos[k], neg[k], losses[k], adversarial=False),
        "apply": lambda k: eng.apply(),
    }
    for name, fn in runs.items():
        for k in range(a.warmup):
            fn(k)
    windows = {name: [] for name in runs}
    for _ in range(WINDOWS):                                   # interleaved: one window of each in turn
        for name, fn in runs.items():
            windows[name].append(_timed(lambda k: fn(a.warmup + k), a.steps))
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(eng.P).all())
    entries = (U + I) * d
    apply_bytes = 4.0 * 8 * entries
    out = {"script": "scripts/bench_apr.py", "shape": a.shape, "users": U, "items": I, "nnz": int(train.nnz), "d": d,
           "batch": B, "steps": a.steps, "warmup": a.warmup, "windows": WINDOWS}
    for name, w in windows.items():
        out[name + "_ms"] = round(_median(w), 4)
        out[name + "_windows"] = [round(x, 4) for x in w]
    out["torch_over_adversarial"] = round(out["torch_ms"] / out["adversarial_ms"], 2)
    out["adversarial_over_mf"] = round(out["adversarial_ms"] / out["mf_ms"], 2)
    out["plain_over_mf"] = round(out["plain_ms"] / out["mf_ms"], 2)
    out["apply_entries"] = entries
    out["apply_bound_ms"] = round(apply_bytes / HBM_BYTES_PER_S * 1e3, 5)
    out["apply_over_bound"] = round(out["apply_ms"] / out["apply_bound_ms"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="gowalla")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    line = json.dumps(bench(args))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
