"""Step times of the IRGAN engine (neurec_amd/irgan.py) at the reference's defaults on gowalla's counts, beside a torch
statement of the same semantics on the same device.

    python scripts/bench_irgan.py [--g-users 200] [--d-steps 200] [--data-users 2048] [--repeats 5] [--torch-g 50]
                                  [--torch-d 100] [--score-users 2048] [--out profiles/r28_irgan.json]

conf/IRGAN.properties: factors_num 20, batch_size 32, d_tau 0.2, d_reg 0.1/16, g_reg 0, lr 0.001.  U = 29,858,
I = 40,981, 813,886 train entries (neurec_amd/synth.py).  In ONE process, `--repeats` windows of engine work and of the
torch statement, INTERLEAVED, each timed between device events after a warm-up: the median window and the range.

    g           us per generator user step: `--g-users` train users in sequence through one C call (4 launches a user)
    d           us per discriminator step: `--d-steps` batches of 32 triples of real D data through one C call
    data        train users per second of d_data() on `--data-users` users (scoring GEMM, weights, draws)
    torch       the same work in eager torch, same sequential order: dense softmax, torch.multinomial, autograd of the
                stated losses, `p -= lr * grad` on the touched tables
    bound       the bytes each path must move over the measured device copy rate: per G user one read and one write of
                Q_g and b_g plus the logits and the weights written and read; per D-data block the score slab once
                (written by the GEMM, read and rewritten as weights, read by the draws: four passes counted)
    score       users / s of score() against P Q^T + b in torch

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

D, BATCH, TAU, LR, G_REG, D_REG = 20, 32, 0.2, 0.001, 0.0, 0.1 / 16


def _median(xs, scale=1.0):
    xs = sorted(x * scale for x in xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def _torch_side(tables, indptr, indices, dev):
    import torch
    T = {k: torch.from_numpy(v).to(dev).requires_grad_() for k, v in tables.items()}
    pos_of = lambda u: torch.from_numpy(indices[indptr[u]:indptr[u + 1]].astype("int64")).to(dev)     # noqa: E731

    def sgd(names, loss):
        grads = torch.autograd.grad(loss, [T[k] for k in names])
        with torch.no_grad():
            for k, g in zip(names, grads):
                T[k] -= LR * g

    def g_step(u):
        pos = pos_of(u)
        with torch.no_grad():
            p = torch.softmax(T["g_Q"] @ T["g_P"][u] + T["g_b"], 0)
            pn = 0.8 * p
            pn[pos] += 0.2 / len(pos)
            s = torch.multinomial(pn, 2 * len(pos), replacement=True)
            x = (T["d_P"][u] * T["d_Q"][s]).sum(1) + T["d_b"][s]
            r = 2 * (torch.sigmoid(x) - 0.5) * p[s] / pn[s]
        logp = torch.log_softmax(T["g_Q"] @ T["g_P"][u] + T["g_b"], 0)
        loss = -(logp[s] * r).mean() + G_REG * ((T["g_P"][u] ** 2).sum() + (T["g_Q"][s] ** 2).sum() +
                                                (T["g_b"][s] ** 2).sum()) / 2
        sgd(("g_P", "g_Q", "g_b"), loss)

    def d_step(users, items, labels):
        x = (T["d_P"][users] * T["d_Q"][items]).sum(1) + T["d_b"][items]
        ce = torch.nn.functional.binary_cross_entropy_with_logits(x, labels, reduction="sum")
        l2 = ((T["d_P"][users] ** 2).sum() + (T["d_Q"][items] ** 2).sum() + (T["d_b"][items] ** 2).sum()) / 2
        sgd(("d_P", "d_Q", "d_b"), ce + len(users) * D_REG * l2)

    def d_data(users, deg_max):
        with torch.no_grad():
            prob = torch.softmax((T["g_P"][users] @ T["g_Q"].t() + T["g_b"]) / TAU, 1)
            return torch.multinomial(prob, deg_max, replacement=True)

    def score(users):
        with torch.no_grad():
            return T["g_P"][users] @ T["g_Q"].t() + T["g_b"]
    return g_step, d_step, d_data, score


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--g-users", type=int, default=200)
    ap.add_argument("--d-steps", type=int, default=200)
    ap.add_argument("--data-users", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-g", type=int, default=50)
    ap.add_argument("--torch-d", type=int, default=100)
    ap.add_argument("--score-users", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_irgan.json"))
    a = ap.parse_args()
    from neurec_amd import synth
    from neurec_amd.irgan import IRGANEngine
    from neurec_amd.model.general_recommender.IRGAN import initial_tables
    train, _ = synth.interactions("gowalla")
    U, I = train.shape
    tables = initial_tables(U, I, D)
    eng = IRGANEngine(tables, train, LR, G_REG, D_REG, TAU, BATCH)
    dev = eng.dev
    rs = np.random.RandomState(0)
    g_users = np.sort(rs.choice(eng.train_users, a.g_users, replace=False)).astype(np.int32)
    data_users = np.sort(rs.choice(eng.train_users, a.data_users, replace=False)).astype(np.int32)
    triples = eng.d_data(users=data_users)
    n_tr = int(triples[0].numel())
    n_d = min(a.d_steps * BATCH, n_tr)
    order = torch.from_numpy(rs.permutation(n_tr)[:n_d].astype(np.int32)).to(dev)
    run_g = lambda k: eng.g_users(g_users)                                       # noqa: E731
    run_d = lambda k: eng._d_run(triples[0], triples[1], triples[2], order, BATCH, None)      # noqa: E731
    run_data = lambda k: eng.d_data(users=data_users)                            # noqa: E731
    for fn in (run_g, run_d, run_data):
        _timed(fn, 1)
    tg, td, tdata, tscore = _torch_side(tables, eng.h_indptr, eng.h_indices, dev)
    tu = torch.from_numpy(data_users.astype(np.int64)).to(dev)
    deg_max = int(eng.h_deg[data_users].max())
    th = tuple(t.cpu() for t in triples)
    batches = [tuple(x[order.cpu().long()[s * BATCH:(s + 1) * BATCH]].to(dev).to(dt)
                     for x, dt in zip(th, (torch.int64, torch.int64, torch.float32))) for s in range(a.torch_d)]
    t_g = lambda k: [tg(int(u)) for u in g_users[:a.torch_g]]                    # noqa: E731
    t_d = lambda k: [td(*b) for b in batches]                                    # noqa: E731
    t_data = lambda k: [tdata(tu[lo:lo + 512], deg_max) for lo in range(0, len(tu), 512)]     # noqa: E731
    for fn in (t_g, t_d, t_data):
        _timed(fn, 1)
    win = {k: [] for k in ("g", "d", "data", "tg", "td", "tdata")}
    for _ in range(a.repeats):                                   # interleaved: all see the same state of the machine
        win["g"].append(_timed(run_g, 1) / len(g_users))
        win["tg"].append(_timed(t_g, 1) / a.torch_g)
        win["d"].append(_timed(run_d, 1) / -(-n_d // BATCH))
        win["td"].append(_timed(t_d, 1) / len(batches))
        win["data"].append(_timed(run_data, 1))
        win["tdata"].append(_timed(t_data, 1))
    # the device copy rate, measured: 256 MiB copied (read + write)
    buf = torch.empty(64 << 20, dtype=torch.float32, device=dev)
    dst = torch.empty_like(buf)
    _timed(lambda k: dst.copy_(buf), 3)
    copy_ms = sorted(_timed(lambda k: dst.copy_(buf), 5) for _ in range(5))[2]
    rate = 2 * buf.numel() * 4 / copy_ms * 1e3
    ld = (I + 63) // 64 * 64
    bytes_g = 4 * (2 * I * D + 2 * I + 2 * I + 2 * I)            # Q and b read and written; z and w written and read
    bytes_data = 4 * 4 * ld * len(data_users)
    g_us, d_us = _median(win["g"], 1e3), _median(win["d"], 1e3)
    data_ms = _median(win["data"])
    out = {"shape": {"users": U, "items": I, "nnz": int(train.nnz), "train_users": int(len(eng.train_users)), "d": D,
                     "batch": BATCH, "d_tau": TAU, "g_users": int(len(g_users)), "mean_deg_g": float(eng.h_deg[g_users].mean()),
                     "d_steps": -(-n_d // BATCH), "data_users": int(len(data_users))},
           "engine": {"g_us_per_user": g_us, "launches_per_user": 4, "d_us_per_step": d_us, "launches_per_d_step": 1,
                      "data_ms": data_ms, "data_users_per_s": len(data_users) / data_ms["median"] * 1e3},
           "torch": {"g_us_per_user": _median(win["tg"], 1e3), "d_us_per_step": _median(win["td"], 1e3),
                     "data_ms": _median(win["tdata"]),
                     "data_users_per_s": len(data_users) / _median(win["tdata"])["median"] * 1e3},
           "bound": {"copy_rate_tb_s": rate / 1e12, "g_bytes_per_user": bytes_g, "g_us": bytes_g / rate * 1e6,
                     "g_over_bound": g_us["median"] / (bytes_g / rate * 1e6), "data_bytes": bytes_data,
                     "data_ms": bytes_data / rate * 1e3, "data_over_bound": data_ms["median"] / (bytes_data / rate * 1e3)}}
    out["engine_over_torch"] = {"g": g_us["median"] / out["torch"]["g_us_per_user"]["median"],
                                "d": d_us["median"] / out["torch"]["d_us_per_step"]["median"],
                                "data": data_ms["median"] / out["torch"]["data_ms"]["median"]}
    n = a.score_users
    su = rs.randint(0, U, n).astype(np.int32)
    sut = torch.from_numpy(su.astype(np.int64)).to(dev)
    _timed(lambda k: eng.score(su), 3)
    sm = sorted(_timed(lambda k: eng.score(su), 5) for _ in range(5))
    _timed(lambda k: tscore(sut), 3)
    tm = sorted(_timed(lambda k: tscore(sut), 5) for _ in range(5))
    out["score"] = {"users": n, "ms": sm[2], "min": sm[0], "max": sm[-1], "users_per_s": n / sm[2] * 1e3,
                    "torch": {"ms": tm[2], "min": tm[0], "max": tm[-1], "users_per_s": n / tm[2] * 1e3}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
