"""Step time and predict() throughput of the SRGNN engine (neurec_amd/srgnn.py) at the reference's defaults on gowalla's
item count, beside a torch-on-device autograd statement of the same step.

    python scripts/bench_srgnn.py [--steps 100] [--warmup 20] [--repeats 5] [--torch-steps 30] [--predict-users 2000]

conf/SRGNN.properties: hidden_size 64, batch_size 100, step 1, L2 1e-5, lr 0.001, hybrid, max_seq_len 200.  I = 40,981.
The sessions are synthetic: 200 items each, uniform over the table — the step's cost depends on their lengths, not on
which ids they are.  In ONE process, `--repeats` windows of `--steps` steps of the engine and of `--torch-steps` steps
of the torch statement, INTERLEAVED, each timed between device events after a warm-up: the median window and the range,
in ms per step.

    engine          ms_per_step (median, min, max), grad_ms / apply_ms (nrhip_srgnn_step alone and the Adam application
                    alone), launches per step
    torch           the same step written with torch ops on the device, fed as the reference feeds it (unique nodes, alias
                    map and the two dense normalised adjacency matrices [B, n, n], built on the host BEFORE the timed
                    window and resident on the device): gathers, batched matmuls, the cell, the readout, the [B, I]
                    logits, cross_entropy, the regulariser over all 14 variables, autograd, torch.optim.Adam
    predict         users / s of score(): the forward pass over resident sequences in batches of batch_size + the [n, I]
                    scores
    bound           the bytes the step must move once over the measured HBM copy rate: the table read for the logits and
                    again for d sess, ApplyAdam's read and write of it (4 sweeps), m and v read and written (2 each), G
                    written and read (2), and the [B, I] logits written once and read twice; and the multiply-adds (the
                    head 3 B I d; per node and iteration 11 d^2 forward, twice that backward) over VALU_RATE

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
D, B, STEP, L, LR, L2 = 64, 100, 1, 200, 0.001, 1e-5


def _feeds(steps, batch, seed=0):
    import numpy as np
    rs = np.random.RandomState(seed)
    return rs.randint(0, N_ITEMS, (steps, batch, L)).astype(np.int32), rs.randint(0, N_ITEMS, (steps, batch)).astype(np.int32)


def _host_graph(seq):
    """SRGNN._build_session_graph for full-length sessions: items [B, n], alias [B, L], A_in, A_out [B, n, n]"""
    import numpy as np
    uniq = [np.unique(row, return_inverse=True) for row in seq]
    n = max(len(u) for u, _ in uniq)
    items = np.full((len(seq), n), N_ITEMS, np.int64)
    alias = np.zeros((len(seq), L), np.int64)
    a_in, a_out = np.zeros((len(seq), n, n), np.float32), np.zeros((len(seq), n, n), np.float32)
    for b, (u, inv) in enumerate(uniq):
        items[b, :len(u)], alias[b] = u, inv
        adj = np.zeros((n, n))
        adj[inv[:-1], inv[1:]] = 1
        s_in, s_out = adj.sum(0), adj.sum(1)
        s_in[s_in == 0] = 1
        s_out[s_out == 0] = 1
        a_in[b], a_out[b] = adj / s_in, adj.T / s_out
    return items, alias, a_in, a_out


def _torch_step_fn(tables):
    import torch
    dev = "cuda"
    P = {k: torch.from_numpy(v).to(dev).requires_grad_() for k, v in tables.items()}
    opt = torch.optim.Adam(list(P.values()), lr=LR, betas=(0.9, 0.999), eps=1e-8)

    def step(items, alias, a_in, a_out, target):
        n_b, n = items.shape
        table = torch.cat([P["embedding"], torch.zeros(1, D, device=dev)])
        h = table[items]
        for _ in range(STEP):
            s = h.reshape(-1, D)
            fi = (s @ P["W_in"] + P["b_in"]).reshape(n_b, n, D)
            fo = (s @ P["W_out"] + P["b_out"]).reshape(n_b, n, D)
            x = torch.cat([a_in @ fi, a_out @ fo], dim=-1).reshape(-1, 2 * D)
            g = torch.sigmoid(torch.cat([x, s], 1) @ P["gates_kernel"] + P["gates_bias"])
            r, u = g[:, :D], g[:, D:]
            c = torch.tanh(torch.cat([x, r * s], 1) @ P["candidate_kernel"] + P["candidate_bias"])
            h = (u * s + (1 - u) * c).reshape(n_b, n, D)
        seq_h = torch.gather(h, 1, alias.unsqueeze(-1).expand(-1, -1, D))
        last = seq_h[:, -1] @ P["nasr_w1"]
        m = torch.sigmoid(last.unsqueeze(1) + seq_h @ P["nasr_w2"] + P["nasr_b"])
        coef = m @ P["nasrv"].t()
        a = (coef * seq_h).sum(1)
        sess = torch.cat([a, last], 1) @ P["B"]
        loss = torch.nn.functional.cross_entropy(sess @ P["embedding"].t(), target)
        loss = loss + L2 * sum((v ** 2).sum() for v in P.values()) / 2
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss
    return step


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=30)
    ap.add_argument("--predict-users", type=int, default=2000)
    a = ap.parse_args()
    from neurec_amd import engine as E
    from neurec_amd.model.sequential_recommender.SRGNN import initial_values
    from neurec_amd.srgnn import SRGNNEngine
    tables = initial_values(N_ITEMS, D)
    eng = SRGNNEngine(tables, LR, L2, B, L, STEP)
    dev = eng.T["embedding"].device
    n_feed = 8
    seq_h, target_h = _feeds(n_feed, B)
    seq, target = torch.from_numpy(seq_h).to(dev), torch.from_numpy(target_h).to(dev)
    loss2 = torch.zeros(2, device=dev)

    def step(k):
        j = k % n_feed
        eng.step(seq[j], target[j], loss2)
    _timed(step, a.warmup)
    tstep = None
    if a.torch_steps:
        fn = _torch_step_fn(tables)
        graphs = [[torch.from_numpy(x).to(dev) for x in _host_graph(seq_h[j])] for j in range(n_feed)]
        t64 = target.long()
        tstep = lambda k: fn(*graphs[k % n_feed], t64[k % n_feed])
        _timed(tstep, 5)
    windows, tw = [], []
    for _ in range(a.repeats):                                   # interleaved: both see the same state of the machine
        windows.append(_timed(step, a.steps))
        if tstep is not None:
            tw.append(_timed(tstep, a.torch_steps))
    windows.sort()
    tw.sort()
    grad_ms = _timed(lambda k: eng.gradients(seq[k % n_feed], target[k % n_feed], loss2), a.steps)
    for g in eng.G.values():
        g.zero_()
    apply_ms = _timed(lambda k: eng.apply(), a.steps)
    launches = {"graph, nodes": 2, "iteration forward": 4 * STEP, "readout": 2, "softmax head": 5, "transposes, readout backward": 3,
                "iteration backward": 5 * STEP, "variable gradients": 2, "sort (3), rows": 4, "loss": 1, "apply": 1}
    out = {"device": E.device_info() if hasattr(E, "device_info") else None,
           "shape": {"n_items": N_ITEMS, "hidden_size": D, "batch_size": B, "step": STEP, "session_length": L, "L2": L2},
           "engine": {"ms_per_step": windows[len(windows) // 2], "min": windows[0], "max": windows[-1],
                      "grad_ms": grad_ms, "apply_ms": apply_ms, "launches_per_step": sum(launches.values()),
                      "launches": launches}}
    if tw:
        out["torch"] = {"ms_per_step": tw[len(tw) // 2], "min": tw[0], "max": tw[-1]}
        out["engine_over_torch"] = out["engine"]["ms_per_step"] / out["torch"]["ms_per_step"]
    n = a.predict_users
    rs = np.random.RandomState(1)
    eng.set_sequences(np.arange(n + 1, dtype=np.int64) * L, rs.randint(0, N_ITEMS, n * L).astype(np.int32))
    users = np.arange(n)
    predict = lambda k: eng.score(users)
    _timed(predict, 2)
    pm = sorted(_timed(predict, 5) for _ in range(3))[1]
    out["predict"] = {"users": n, "ms": pm, "users_per_s": n / pm * 1e3}
    table = N_ITEMS * D
    nbytes = ((4 + 2 + 2 + 2) * table + 3 * B * N_ITEMS) * 4
    macs = 3 * B * N_ITEMS * D + 3 * STEP * B * L * 11 * D * D
    out["bound"] = {"bytes": nbytes, "hbm_ms": nbytes / HBM_RATE * 1e3, "multiply_adds": macs,
                    "valu_ms": macs / VALU_RATE * 1e3, "bytes_per_flop": nbytes / (2.0 * macs)}
    out["bound"]["bound_ms"] = max(out["bound"]["valu_ms"], out["bound"]["hbm_ms"])
    out["step_over_bound"] = out["engine"]["ms_per_step"] / out["bound"]["bound_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
