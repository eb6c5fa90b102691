"""Step time and predict() throughput of the SASRec engine (neurec_amd/sasrec.py) at the reference's defaults on
gowalla's item count, beside a torch-on-device autograd statement of the same step.

    python scripts/bench_sasrec.py [--steps 200] [--warmup 30] [--repeats 5] [--batch 128] [--torch-steps 100]
                                   [--predict-users 2048]

conf/SASRec.properties: hidden_units 50, max_len 50, num_blocks 2, num_heads 1, batch 128, dropout 0.5, lr 0.001,
l2_emb 0.  I = 40,981.  The rows are synthetic: per row a length drawn uniformly from 1..max_len (pre-padded), items,
positives and negatives uniform over the table — the step's cost does not depend on which ids they are.  In ONE
process, `--repeats` windows of `--steps` steps, timed between device events after `--warmup` steps: the median window
and the range, in ms per step.

    engine          ms_per_step (median, min, max), grad_ms / apply_ms (nrhip_sasrec_step alone and the Adam
                    applications alone: launch-bound loops, not a split), launches per step
    torch           the same step written with torch ops on the device (gathers, layer_norm restated with the biased
                    variance and eps inside the root, matmuls, masked softmax, the loss as written, autograd, and
                    torch.optim.Adam(beta2 0.98) — dense on every variable, so the sweep of the item table is in it as
                    it is in the engine's ApplyAdam); dropout through torch's own generator
    predict         users / s of score(): forward with training off + the [n, I] scores
    bound           the step's multiply-adds (the linear layers: 5 products of [R, d] x [d, d] per block forward, twice
                    that backward; the attention: 2 R L d forward, 4 R L d backward; R = B L rows) over VALU_RATE, and the
                    bytes the step must move once (the item table's gradient, two slots and the variable: ApplyAdam's
                    4 reads + 3 writes of I d floats; the activations are L2-resident) over the measured HBM copy rate;
                    bound_ms is the larger, and bytes_per_flop = bytes / (2 multiply-adds)

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
HBM_RATE = 6.29e12
N_ITEMS = 40981
D, L, NB, H, RATE, LR = 50, 50, 2, 1, 0.5, 0.001


def _tables(n_items):
    import numpy as np
    from neurec_amd.util.tool import get_initializer
    embed, kernel = get_initializer("xavier_uniform", 0.01, seed=2017), get_initializer("xavier_uniform", 0.01, seed=2018)
    z, o = (lambda: np.zeros(D, np.float32)), (lambda: np.ones(D, np.float32))
    item, pos = embed([n_items, D]), embed([L, D])
    blocks = [[z(), o(), kernel([D, D]), z(), kernel([D, D]), z(), kernel([D, D]), z(), z(), o(), kernel([D, D]), z(),
               kernel([D, D]), z()] for _ in range(NB)]
    return item, pos, blocks, (z(), o())


def _feeds(n_items, steps, batch, seed=0):
    import numpy as np
    rs = np.random.RandomState(seed)
    seq, pos, neg = (np.full((steps, batch, L), n_items, np.int32) for _ in range(3))
    lens = rs.randint(1, L + 1, (steps, batch))
    real = np.arange(L)[None, None, :] >= (L - lens)[:, :, None]
    for a in (seq, pos, neg):
        a[real] = rs.randint(0, n_items, int(real.sum()))
    return seq, pos, neg


def _torch_step_fn(tables, n_items):
    """the step as torch ops + autograd + torch.optim.Adam; returns fn(seq, pos, neg) on device int64 tensors"""
    import torch
    dev = "cuda"
    item, pe, blocks, lnf = tables
    P = [torch.from_numpy(item).to(dev).requires_grad_(), torch.from_numpy(pe).to(dev).requires_grad_()]
    B_ = [[torch.from_numpy(t).to(dev).requires_grad_() for t in blk] for blk in blocks]
    F = [torch.from_numpy(t).to(dev).requires_grad_() for t in lnf]
    params = P + [t for blk in B_ for t in blk] + F
    opt = torch.optim.Adam(params, lr=LR, betas=(0.9, 0.98), eps=1e-8)
    sd = float(D) ** 0.5
    tril = torch.tril(torch.ones(L, L, device=dev, dtype=torch.bool))
    pad_val = float(-2 ** 32 + 1)
    drop = torch.nn.functional.dropout

    def ln(x, beta, gamma):
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        return gamma * ((x - mu) / (var + 1e-8) ** 0.5) + beta

    def step(seq, pos, neg):
        table = torch.cat([P[0], torch.zeros(1, D, device=dev)]) * sd
        mask = (seq != n_items).unsqueeze(-1).float()
        x = drop(table[seq] + P[1], RATE) * mask
        for b in B_:
            q = ln(x, b[0], b[1])
            Q, K, V = q @ b[2] + b[3], x @ b[4] + b[5], x @ b[6] + b[7]
            split = lambda t: torch.cat(torch.split(t, D // H, dim=2), dim=0)
            Q_, K_, V_ = split(Q), split(K), split(V)
            w = Q_ @ K_.transpose(1, 2) / (D // H) ** 0.5
            kmask = (x.sum(-1) != 0).repeat(H, 1).unsqueeze(1) & tril
            w = torch.softmax(torch.where(kmask, w, torch.full_like(w, pad_val)), dim=-1)
            w = drop(w * (q.sum(-1) != 0).float().repeat(H, 1).unsqueeze(-1), RATE)
            y = torch.cat(torch.split(w @ V_, seq.shape[0], dim=0), dim=2) + q
            u = ln(y, b[8], b[9])
            f = drop(drop(torch.relu(u @ b[10] + b[11]), RATE) @ b[12] + b[13], RATE)
            x = (f + u) * mask
        z = ln(x, F[0], F[1])
        it = (pos != n_items).float()
        lp, ln_ = (table[pos] * z).sum(-1), (table[neg] * z).sum(-1)
        loss = ((-torch.log(torch.sigmoid(lp) + 1e-24) - torch.log(1 - torch.sigmoid(ln_) + 1e-24)) * it).sum() / it.sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss
    return step


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--torch-steps", type=int, default=100)
    ap.add_argument("--predict-users", type=int, default=2048)
    a = ap.parse_args()
    from neurec_amd import engine as E
    from neurec_amd.sasrec import SASRecEngine
    tables = _tables(N_ITEMS)
    eng = SASRecEngine(tables[0], tables[1], tables[2], tables[3], LR, 0.0, a.batch, H, RATE)
    dev = eng.item_emb.device
    n_feed = 32
    seq, pos, neg = (torch.from_numpy(x).to(dev) for x in _feeds(N_ITEMS, n_feed, a.batch))
    counts = [int((pos[k] != N_ITEMS).sum().item()) for k in range(n_feed)]
    loss2 = torch.zeros(2, device=dev)

    def step(k):
        j = k % n_feed
        eng.step(seq[j], pos[j], neg[j], loss2, None, counts[j])
    _timed(step, a.warmup)
    windows = sorted(_timed(step, a.steps) for _ in range(a.repeats))
    grad_ms = _timed(lambda k: eng.gradients(seq[k % n_feed], pos[k % n_feed], neg[k % n_feed], loss2), a.steps)
    for g in eng.G.values():
        g.zero_()
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    launches = 3 + 2 + NB * 9 + 1 + NB * (1 + 2 * 5 + 2 * 2 + 3 + 5 + 2) + 4
    out = {"device": E.device_info() if hasattr(E, "device_info") else None,
           "shape": {"n_items": N_ITEMS, "hidden_units": D, "max_len": L, "num_blocks": NB, "num_heads": H,
                     "batch": a.batch, "dropout_rate": RATE},
           "engine": {"ms_per_step": windows[len(windows) // 2], "min": windows[0], "max": windows[-1],
                      "grad_ms": grad_ms, "apply_ms": apply_ms, "launches_per_step_about": launches}}
    if a.torch_steps:
        fn = _torch_step_fn(tables, N_ITEMS)
        s64, p64, n64 = seq.long(), pos.long(), neg.long()
        tstep = lambda k: fn(s64[k % n_feed], p64[k % n_feed], n64[k % n_feed])
        _timed(tstep, max(a.warmup // 3, 5))
        tw = sorted(_timed(tstep, a.torch_steps) for _ in range(min(a.repeats, 3)))
        out["torch"] = {"ms_per_step": tw[len(tw) // 2], "min": tw[0], "max": tw[-1]}
        out["engine_over_torch"] = out["engine"]["ms_per_step"] / out["torch"]["ms_per_step"]
    # predict(): every user's last L items — here the feeds' rows
    n = a.predict_users
    rows = torch.from_numpy(_feeds(N_ITEMS, 1, n, seed=1)[0][0]).to(dev)

    predict = lambda k: eng.score_rows(rows)
    _timed(predict, 3)
    pm = sorted(_timed(predict, 10) for _ in range(3))[1]
    out["predict"] = {"users": n, "ms": pm, "users_per_s": n / pm * 1e3}
    R = a.batch * L
    macs = NB * (15 * R * D * D + 6 * R * L * D)
    nbytes = 7 * N_ITEMS * D * 4
    out["bound"] = {"multiply_adds": macs, "valu_ms": macs / VALU_RATE * 1e3, "bytes": nbytes,
                    "hbm_ms": nbytes / HBM_RATE * 1e3, "bytes_per_flop": nbytes / (2.0 * macs)}
    out["bound"]["bound_ms"] = max(out["bound"]["valu_ms"], out["bound"]["hbm_ms"])
    out["step_over_bound"] = out["engine"]["ms_per_step"] / out["bound"]["bound_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
