"""Step time and predict() throughput of the Caser engine (neurec_amd/caser.py) at the reference's defaults on gowalla's
user and item counts, beside a torch-on-device autograd statement of the same step.

    python scripts/bench_caser.py [--steps 200] [--warmup 30] [--repeats 5] [--batch 256] [--torch-steps 100]
                                  [--predict-users 2048]

conf/Caser.properties: factors_num 50, seq_L 5, seq_T 3, nv 4, nh 16, neg_samples 3, batch 256, dropout 0.5, lr 0.001,
l2_reg 0.001.  U = 29,858, I = 40,981.  The rows are synthetic: users, items, positives and negatives uniform over
their tables, one row in eight front-padded — the step's cost does not depend on which ids they are.  In ONE process,
`--repeats` windows of `--steps` steps of the engine and of `--torch-steps` steps of the torch statement, INTERLEAVED,
each timed between device events after a warm-up: the median window and the range, in ms per step.

    engine          ms_per_step (median, min, max), grad_ms / apply_ms (nrhip_caser_step alone and the Adam application
                    alone: launch-bound loops, not a split), launches per step
    torch           the same step written with torch ops on the device (gathers, conv2d, amax, dropout, matmuls, the
                    loss as written, the regulariser, autograd, torch.optim.Adam — dense on every variable, so the
                    sweeps of the four tables are in it as they are in the engine's ApplyAdam)
    predict         users / s of score(): forward with training off + the [n, I] scores
    bound           the step's multiply-adds per row (vertical L nv d; horizontal d nh sum_i i (L - i + 1); dense F d;
                    logits (T + N) 2 d; backward: dense twice, the saved windows d nh L (L + 1) twice, logits twice)
                    over VALU_RATE, and the bytes the step must move once (the regulariser's sweep of the four tables,
                    1 read + 1 read-modify-write, and ApplyAdam's 4 reads + 3 writes of them) over the measured HBM
                    copy rate; bound_ms is the larger, and bytes_per_flop = bytes / (2 multiply-adds)

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
N_USERS, N_ITEMS = 29858, 40981
D, L, T, N, NV, NH, RATE, LR, L2 = 50, 5, 3, 3, 4, 16, 0.5, 0.001, 0.001
F = NV * D + NH * L


def _tables():
    import numpy as np
    from neurec_amd.caser import table_names
    from neurec_amd.util.tool import get_initializer
    embed, dense = get_initializer("xavier_uniform", 0.01, seed=2017), get_initializer("xavier_uniform", 0.01, seed=2019)
    conv = get_initializer("uniform", 0.1, seed=2018)
    values = [embed([N_USERS, D]), embed([N_ITEMS, D]), embed([N_ITEMS, 2 * D]), np.zeros(N_ITEMS, np.float32),
              conv([L, NV]), np.zeros(NV, np.float32)]
    for i in range(1, L + 1):
        values += [conv([i, D, NH]), np.zeros(NH, np.float32)]
    values += [dense([F, D]), np.zeros(D, np.float32)]
    return dict(zip(table_names(L), values))


def _feeds(steps, batch, seed=0):
    import numpy as np
    rs = np.random.RandomState(seed)
    users = rs.randint(0, N_USERS, (steps, batch)).astype(np.int32)
    seq = rs.randint(0, N_ITEMS, (steps, batch, L)).astype(np.int32)
    pads = np.where(rs.rand(steps, batch) < 0.125, rs.randint(1, L + 1, (steps, batch)), 0)
    seq[np.arange(L)[None, None, :] < pads[:, :, None]] = N_ITEMS
    return users, seq, rs.randint(0, N_ITEMS, (steps, batch, T)).astype(np.int32), \
        rs.randint(0, N_ITEMS, (steps, batch, N)).astype(np.int32)


def _torch_step_fn(tables):
    """the step as torch ops + autograd + torch.optim.Adam; returns fn(users, seq, pos, neg) on device int64 tensors"""
    import torch
    dev = "cuda"
    P = {k: torch.from_numpy(v).to(dev).requires_grad_() for k, v in tables.items()}
    opt = torch.optim.Adam(list(P.values()), lr=LR, betas=(0.9, 0.999), eps=1e-8)
    conv2d = torch.nn.functional.conv2d

    def step(users, seq, pos, neg):
        B = seq.shape[0]
        table = torch.cat([P["seq_item_embeddings"], torch.zeros(1, D, device=dev)])
        img = table[seq].unsqueeze(1)                                             # (b, 1, L, d)
        out_v = conv2d(img, P["conv_v_kernel"].t().reshape(NV, 1, L, 1), P["conv_v_bias"])      # (b, nv, 1, d)
        feats = [out_v.squeeze(2).transpose(1, 2).reshape(B, NV * D)]             # feature j nv + c
        for i in range(1, L + 1):
            k = P["conv_h%d_kernel" % i].permute(2, 0, 1).unsqueeze(1)            # (nh, 1, i, d)
            feats.append(torch.relu(conv2d(img, k, P["conv_h%d_bias" % i])).squeeze(3).amax(dim=2))
        x = torch.nn.functional.dropout(torch.cat(feats, dim=1), RATE)
        z = torch.relu(x @ P["fc1_kernel"] + P["fc1_bias"])
        p = torch.cat([z, P["user_embeddings"][users]], dim=1)
        tar = torch.cat([pos, neg], dim=1)
        logits = (P["item_embeddings"][tar] * p.unsqueeze(1)).sum(-1) + P["item_biases"][tar]
        lp, ln_ = logits[:, :T], logits[:, T:]
        loss = (-torch.log(torch.sigmoid(lp) + 1e-24)).mean() + (-torch.log(1 - torch.sigmoid(ln_) + 1e-24)).mean()
        loss = loss + L2 * sum((P[k] ** 2).sum() for k in ("user_embeddings", "seq_item_embeddings", "item_embeddings",
                                                           "item_biases")) / 2
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--torch-steps", type=int, default=100)
    ap.add_argument("--predict-users", type=int, default=2048)
    a = ap.parse_args()
    from neurec_amd import engine as E
    from neurec_amd.caser import CaserEngine
    tables = _tables()
    eng = CaserEngine(tables, LR, L2, a.batch, T, N, NV, NH, RATE)
    dev = eng.item_embeddings.device
    n_feed = 32
    users, seq, pos, neg = (torch.from_numpy(x).to(dev) for x in _feeds(n_feed, a.batch))
    loss2 = torch.zeros(2, device=dev)

    def step(k):
        j = k % n_feed
        eng.step(users[j], seq[j], pos[j], neg[j], loss2)
    _timed(step, a.warmup)
    tstep = None
    if a.torch_steps:
        fn = _torch_step_fn(tables)
        u64, s64, p64, n64 = users.long(), seq.long(), pos.long(), neg.long()
        tstep = lambda k: fn(u64[k % n_feed], s64[k % n_feed], p64[k % n_feed], n64[k % n_feed])
        _timed(tstep, max(a.warmup // 3, 5))
    windows, tw = [], []
    for _ in range(a.repeats):                                   # interleaved: both see the same state of the machine
        windows.append(_timed(step, a.steps))
        if tstep is not None:
            tw.append(_timed(tstep, a.torch_steps))
    windows.sort()
    tw.sort()
    grad_ms = _timed(lambda k: eng.gradients(users[k % n_feed], seq[k % n_feed], pos[k % n_feed], neg[k % n_feed],
                                             loss2), a.steps)
    for g in eng.G.values():
        g.zero_()
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    launches = {"nrhip_caser_step": 7, "apply": 1}               # row, wgrad, reduce, sort, rows, l2, loss; ApplyAdam x 18
    out = {"device": E.device_info() if hasattr(E, "device_info") else None,
           "shape": {"n_users": N_USERS, "n_items": N_ITEMS, "factors_num": D, "seq_L": L, "seq_T": T, "neg_samples": N,
                     "nv": NV, "nh": NH, "batch": a.batch, "dropout": RATE, "l2_reg": L2},
           "engine": {"ms_per_step": windows[len(windows) // 2], "min": windows[0], "max": windows[-1],
                      "grad_ms": grad_ms, "apply_ms": apply_ms, "launches_per_step": sum(launches.values()),
                      "launches": launches}}
    if tw:
        out["torch"] = {"ms_per_step": tw[len(tw) // 2], "min": tw[0], "max": tw[-1]}
        out["engine_over_torch"] = out["engine"]["ms_per_step"] / out["torch"]["ms_per_step"]
    n = a.predict_users
    pu, ps, _, _ = _feeds(1, n, seed=1)
    pu, ps = torch.from_numpy(pu[0]).to(dev), torch.from_numpy(ps[0]).to(dev)
    big = CaserEngine(tables, LR, L2, min(n, 4096), T, N, NV, NH, RATE)

    predict = lambda k: big.score_rows(pu, ps)
    _timed(predict, 3)
    pm = sorted(_timed(predict, 10) for _ in range(3))[1]
    out["predict"] = {"users": n, "ms": pm, "users_per_s": n / pm * 1e3}
    fwd = L * NV * D + D * NH * sum(i * (L - i + 1) for i in range(1, L + 1)) + F * D + (T + N) * 2 * D
    bwd = 2 * F * D + 2 * D * NH * L * (L + 1) // 2 + 2 * L * NV * D + 2 * (T + N) * 2 * D
    macs = a.batch * (fwd + bwd)
    table_floats = N_USERS * D + N_ITEMS * (3 * D + 1)
    nbytes = (3 + 7) * table_floats * 4
    out["bound"] = {"multiply_adds": macs, "valu_ms": macs / VALU_RATE * 1e3, "bytes": nbytes,
                    "hbm_ms": nbytes / HBM_RATE * 1e3, "bytes_per_flop": nbytes / (2.0 * macs)}
    out["bound"]["bound_ms"] = max(out["bound"]["valu_ms"], out["bound"]["hbm_ms"])
    out["step_over_bound"] = out["engine"]["ms_per_step"] / out["bound"]["bound_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
