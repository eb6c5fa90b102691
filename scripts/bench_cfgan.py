"""Step times and score() throughput of the CFGAN engine (neurec_amd/cfgan.py) at the reference's defaults on gowalla's
counts, beside a torch-autograd statement of the same steps on the same device.

    python scripts/bench_cfgan.py [--steps 60] [--warmup 10] [--repeats 5] [--torch-steps 30] [--score-users 2048]
                                  [--mode userBased] [--out profiles/r27_cfgan.json]

conf/CFGAN.properties: hiddenLayer_G [400], hiddenLayer_D [125], batches of 32 (G) and 64 (D) rows, ratios 0.7, Adam at
1e-4, reg_G 0.001, reg_D 0.  U = 29,858, I = 40,981, 813,886 train entries (neurec_amd/synth.py).  In ONE process,
`--repeats` windows of `--steps` engine steps and of `--torch-steps` steps of the torch statement, INTERLEAVED, each timed
between device events after a warm-up: the median window and the range, in ms per step, the D step and the G step apart.

    engine      d_ms / g_ms: masks built on the device, the gradient call, the optimiser pass; masks_ms, d_grad_ms,
                g_grad_ms, d_apply_ms, g_apply_ms: each alone (loops of their own, not a split)
    torch       the same steps on dense rows and dense masks made beforehand (the torch side builds none): matmuls,
                the losses with their regularisers, autograd, torch.optim.Adam per network
    bound       the bytes a step must move by the reference's semantics: the optimiser's pass over every variable of the
                stepped network (var, m, v, gradient: 4 reads + 4 writes per float), one write of the gradient, and the
                reads of the kernels the pass runs through (Wg2 and Wd1[n:] once per product with them), over the
                measured HBM copy rate
    score       users / s of score() in --mode against G(R) in torch for the same users (itemBased: the whole G(R), as
                the reference computes it, per user)

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
HG, HD, BATCH_G, BATCH_D = [400], [125], 32, 64
LR, REG_G, REG_D, RATIO, ZR_COEF = 1e-4, 0.001, 0.0, 0.7, 0.03


def _torch_steps(tables):
    """(d_step, g_step)(c, zr, pm) on dense float rows and masks: the graph of CFGAN.py:57-95 with torch ops"""
    import torch
    P = {k: torch.from_numpy(v).to("cuda").requires_grad_() for k, v in tables.items()}
    gen, dis = [k for k in P if k.startswith("gen")], [k for k in P if k.startswith("dis")]
    opt_g = torch.optim.Adam([P[k] for k in gen], lr=LR, betas=(0.9, 0.999), eps=1e-8)
    opt_d = torch.optim.Adam([P[k] for k in dis], lr=LR, betas=(0.9, 0.999), eps=1e-8)
    sp = torch.nn.functional.softplus

    def G(c):
        return torch.sigmoid(c @ P["gen_h0_kernel"] + P["gen_h0_bias"]) @ P["gen_out_kernel"] + P["gen_out_bias"]

    def D(x):
        return torch.sigmoid(x @ P["dis_h0_kernel"] + P["dis_h0_bias"]) @ P["dis_out_kernel"] + P["dis_out_bias"]

    def l2(names):
        return sum((P[k] * P[k]).sum() for k in names) / 2

    def d_step(c, zr, pm):
        fake, real = D(torch.cat([c, G(c) * pm], 1)), D(torch.cat([c, c], 1))
        loss = sp(-real).mean() + sp(fake).mean() + REG_D * l2(dis)
        opt_d.zero_grad(set_to_none=True)
        opt_g.zero_grad(set_to_none=True)
        loss.backward(inputs=[P[k] for k in dis])
        opt_d.step()
        return loss

    def g_step(c, zr, pm):
        out = G(c)
        loss = sp(-D(torch.cat([c, out * pm], 1))).mean() + REG_G * l2(gen) + ZR_COEF * (out * out * zr).sum(1).mean()
        opt_d.zero_grad(set_to_none=True)
        opt_g.zero_grad(set_to_none=True)
        loss.backward(inputs=[P[k] for k in gen])
        opt_g.step()
        return loss
    return d_step, g_step, G


def _median(xs):
    xs = sorted(xs)
    return {"ms_per_step": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=30)
    ap.add_argument("--score-users", type=int, default=2048)
    ap.add_argument("--mode", default="userBased")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_cfgan.json"))
    a = ap.parse_args()
    from neurec_amd import synth
    from neurec_amd.cfgan import CFGANEngine
    from neurec_amd.model.general_recommender.CFGAN import initial_variables
    train, _ = synth.interactions("gowalla")
    U, I = train.shape
    n_rows, n_cols = (I, U) if a.mode == "itemBased" else (U, I)
    tables = initial_variables(n_cols, HG, HD)
    eng = CFGANEngine(tables, train, HG, HD, LR, LR, REG_G, REG_D, RATIO, RATIO, ZR_COEF, BATCH_G, BATCH_D, mode=a.mode)
    dev = eng.dev
    rs = np.random.RandomState(0)
    n_feed = 16
    feeds_d = [rs.choice(n_rows, BATCH_D, replace=False).astype(np.int32) for _ in range(n_feed)]
    feeds_g = [rs.choice(n_rows, BATCH_G, replace=False).astype(np.int32) for _ in range(n_feed)]
    loss3 = torch.zeros(3, device=dev)
    d_step = lambda k: eng.d_step(feeds_d[k % n_feed], loss3)       # noqa: E731
    g_step = lambda k: eng.g_step(feeds_g[k % n_feed], loss3)       # noqa: E731
    _timed(d_step, a.warmup)
    _timed(g_step, a.warmup)
    td = tg = None
    if a.torch_steps:
        fd, fg, _ = _torch_steps(tables)
        R = train.T.tocsr() if a.mode == "itemBased" else train.tocsr()

        def dense(feeds):
            out = []
            for f in feeds:
                zr, pm = eng.masks(f).dense()
                out.append(tuple(torch.from_numpy(np.asarray(x, np.float32)).to(dev)
                                 for x in (np.asarray(R[f].todense()), zr, pm)))
            return out
        bd, bg = dense(feeds_d), dense(feeds_g)
        td = lambda k: fd(*bd[k % n_feed])                           # noqa: E731
        tg = lambda k: fg(*bg[k % n_feed])                           # noqa: E731
        _timed(td, 5)
        _timed(tg, 5)
    win = {"d": [], "g": [], "td": [], "tg": []}
    for _ in range(a.repeats):                                   # interleaved: all see the same state of the machine
        win["d"].append(_timed(d_step, a.steps))
        win["g"].append(_timed(g_step, a.steps))
        if td is not None:
            win["td"].append(_timed(td, a.torch_steps))
            win["tg"].append(_timed(tg, a.torch_steps))
    masks_ms = _timed(lambda k: eng.masks(feeds_d[k % n_feed]), a.steps)
    md = [eng.masks(f) for f in feeds_d]
    mg = [eng.masks(f) for f in feeds_g]
    d_grad = _timed(lambda k: eng._gradients("d", feeds_d[k % n_feed], loss3, md[k % n_feed]), a.steps)
    g_grad = _timed(lambda k: eng._gradients("g", feeds_g[k % n_feed], loss3, mg[k % n_feed]), a.steps)
    for g in eng.G.values():
        g.zero_()
    d_apply = _timed(lambda k: eng.dis.apply(REG_D, eng._partials, loss3[2:3]), a.steps)
    g_apply = _timed(lambda k: eng.gen.apply(REG_G, eng._partials, loss3[1:2]), a.steps)
    n_g = sum(t.numel() for t in eng.gen.T.values())
    n_d = sum(t.numel() for t in eng.dis.T.values())
    wg2, wd_bot = HG[-1] * n_cols, n_cols * HD[0]
    bytes_d = 4 * (8 * n_d + wd_bot + wg2 + wd_bot)              # apply, dWd1[n:] written, Wg2 and Wd1[n:] read forward
    bytes_g = 4 * (8 * n_g + wg2 + 2 * wg2 + 2 * wd_bot)          # apply, dWg2 written, Wg2 and Wd1[n:] read twice
    out = {"mode": a.mode,
           "shape": {"n_rows": n_rows, "n_cols": n_cols, "nnz": int(train.nnz), "hiddenLayer_G": HG, "hiddenLayer_D": HD,
                     "batch_G": BATCH_G, "batch_D": BATCH_D, "floats_G": n_g, "floats_D": n_d},
           "engine": {"d": _median(win["d"]), "g": _median(win["g"]), "masks_ms": masks_ms, "d_grad_ms": d_grad,
                      "g_grad_ms": g_grad, "d_apply_ms": d_apply, "g_apply_ms": g_apply}}
    if td is not None:
        out["torch"] = {"d": _median(win["td"]), "g": _median(win["tg"])}
        out["engine_over_torch"] = {k: out["engine"][k]["ms_per_step"] / out["torch"][k]["ms_per_step"] for k in "dg"}
    out["bound"] = {"d_bytes": bytes_d, "g_bytes": bytes_g, "d_hbm_ms": bytes_d / HBM_RATE * 1e3,
                    "g_hbm_ms": bytes_g / HBM_RATE * 1e3}
    for k, nb, ap_ms in (("d", bytes_d, d_apply), ("g", bytes_g, g_apply)):
        ms = out["engine"][k]["ms_per_step"]
        out["bound"][k + "_reached_tb_s"] = nb / ms / 1e9
        out["bound"][k + "_apply_reached_tb_s"] = 4 * 8 * (n_d if k == "d" else n_g) / ap_ms / 1e9

    n = a.score_users
    su = rs.randint(0, U, n).astype(np.int32)
    score = lambda k: eng.score(su)                                 # noqa: E731
    _timed(score, 3)
    sm = sorted(_timed(score, 5) for _ in range(5))
    out["score"] = {"users": n, "ms": sm[2], "min": sm[0], "max": sm[-1], "users_per_s": n / sm[2] * 1e3,
                    "full_eval_ms": U / (n / sm[2])}
    if a.torch_steps:
        _, _, G = _torch_steps(tables)
        R = train.T.tocsr() if a.mode == "itemBased" else train.tocsr()
        with torch.no_grad():
            if a.mode == "userBased":
                c = torch.from_numpy(np.asarray(R[su].todense(), np.float32)).to(dev)
                fn, per = (lambda k: G(c)), n
            else:                                                # the whole G(R), in row blocks of 4096
                blocks = [torch.from_numpy(np.asarray(R[lo:lo + 4096].todense(), np.float32)).to(dev)
                          for lo in range(0, n_rows, 4096)]
                fn, per = (lambda k: [G(b) for b in blocks]), U
            _timed(fn, 2)
            tm = sorted(_timed(fn, 3) for _ in range(5))
        out["score"]["torch"] = {"users": per, "ms": tm[2], "min": tm[0], "max": tm[-1], "users_per_s": per / tm[2] * 1e3}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
