"""The planned batch-rows forward hop (spmm_wanted_planned_kernel, run from the per-batch work lists
nrhip_spmm_wanted_epoch_plan makes for a whole epoch in one launch) against the hop that finds its rows itself
(spmm_wanted_wave_kernel, NEUREC_SPMM_WANTED_PLANNED=0) and against the full product — bit for bit:
  * the hop alone, gowalla-shaped and random graphs, d = 64, the layer terms of L = 1, 2, 3, B = 1 .. 4096, first, middle
    and short last batch of an epoch: Esum_rows on the batch rows, row_flag and batch_rows under torch.equal; the work
    lists themselves against the host statement of the planner (tests/hostcheck/wantedplancheck.cpp), byte for byte;
  * 50 training steps across an epoch boundary (where the lists are rebuilt): trained tables under torch.equal.
LightGCN.py:132-149 is what the hop computes; only the rows of the batch are read by the loss (LightGCN.py:99-104)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gowalla():
    from neurec_amd import synth
    from neurec_amd.graph import lightgcn_adjacency
    train, _ = synth.interactions_around_test(
        synth.load_test_split(os.path.join(ROOT, "tests", "golden", "gowalla_test_split.npz")), 810128, seed=2018)
    U, I = train.shape
    coo = train.tocoo()
    return lightgcn_adjacency(coo.row, coo.col, U, I, "pre"), train.tocsr(), U, I


def _random(seed, U=1500, I=1200):
    """interactions with hub items (several rows of > 512 and > 64 non-zeros) and users of 1 .. 300 items"""
    from neurec_amd.graph import lightgcn_adjacency
    rng = np.random.RandomState(seed)
    pop = 1.0 / (1.0 + np.arange(I)) ** 0.9
    pop /= pop.sum()
    deg = np.minimum(1 + (rng.pareto(1.2, U) * 8).astype(np.int64), 300)
    rows = np.repeat(np.arange(U), deg)
    cols = np.concatenate([rng.choice(I, k, replace=False, p=pop) for k in deg])
    train = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(U, I))
    return lightgcn_adjacency(rows, cols, U, I, "pre"), train, U, I


def _hostplan():
    d = os.path.join(ROOT, "tests", "hostcheck")
    so, src = os.path.join(d, "libwantedplancheck.so"), os.path.join(d, "wantedplancheck.cpp")
    csrc = os.path.join(ROOT, "neurec_amd", "csrc")
    hdrs = [os.path.join(csrc, "spmm_wanted_plan.h"), os.path.join(csrc, "spmm_blocked_plan.h")]
    if (not os.path.isfile(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", csrc, "-o", so, src])
    lib = C.CDLL(so)
    lib.wp_plan_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_int64)]
    lib.wp_plan_batch.restype = C.c_int64
    return lib


def _epoch_batches(trc, U, I, B, max_batches=2000):
    """the batches of one epoch of the sampler, tagged the way BprEpochSampler.batches() tags them; an epoch of more
    than max_batches batches (B = 1 on 810 k interactions) is cut there, with a short last batch when B > 1"""
    from neurec_amd import engine as E
    from neurec_amd.trainer import BprEpochSampler, TripletBatch
    sampler = BprEpochSampler(trc, I, batch_size=B, seed=2018 + B, plan_users=U)
    if len(sampler) <= max_batches:
        return list(sampler.batches()), sampler._plan[:3 * sampler.n_local]
    users, pos, neg = sampler.sample_epoch()
    n = max_batches * B - B // 2
    plans = E.bpr_plan(users[:n], pos[:n], neg[:n], B, U)
    out = []
    for k in range(max_batches):
        b, e = k * B, min((k + 1) * B, n)
        plan = plans[3 * b:3 * e]
        plan.epoch_plans, plan.batch_index = (plans, B, 1), k
        out.append(TripletBatch(users[b:e], pos[b:e], neg[b:e], plan))
    return out, plans


def _hop_case(A, train, U, I, batches, seed):
    import torch
    from neurec_amd import engine as E
    N, d = U + I, 64
    csr = E.SpmmCSR.from_scipy(A, split_row=U)
    assert csr.ensure_schedule(d)
    hop = E.EpochHopSchedule(csr, d)
    assert hop.ok, "the planned form must exist for this matrix"
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    X, S, La, Lb = (torch.randn(N, d, generator=g, device="cuda") for _ in range(4))
    Y = torch.empty(N, d, device="cuda")
    csr.matmul(X, out=Y)                                                      # the full product
    trc = E.DeviceCSR.from_scipy(train)
    host = _hostplan()
    indptr = np.ascontiguousarray(A.indptr, np.int64)
    for B in batches:
        all_b, keys_dev = _epoch_batches(trc, U, I, B)
        picks = sorted({0, len(all_b) // 2, len(all_b) - 1})                   # the last one is the short batch
        for layers in ((None, None), (La, None), (La, Lb)):                    # the layer terms at L = 1, 2, 3
            for k in picks:
                bu, bp, bn = all_b[k]
                nb = bu.numel()
                where = hop.for_batch(all_b[k].plan, nb)
                assert where is not None
                outs = []
                for planned in (False, True):
                    out = torch.full((N, d), 7.0, device="cuda")
                    flag = torch.zeros(N, dtype=torch.uint8, device="cuda")
                    rows = torch.full((3 * nb,), -1, dtype=torch.int32, device="cuda")
                    args = [csr.plan, E._ptr(csr.indices), E._ptr(csr.vals), E._ptr(X), d, E._ptr(S),
                            E._ptr(layers[0], allow_none=True), E._ptr(layers[1], allow_none=True), E._ptr(out),
                            E._ptr(bu), E._ptr(bp), E._ptr(bn), nb, U, E._ptr(flag), E._ptr(rows)]
                    if planned:
                        E.call("nrhip_spmm_csr_wanted_planned", *args, C.c_void_p(where[0]), where[1], E._stream())
                    else:
                        E.call("nrhip_spmm_csr_wanted_batch", *args, E._stream())
                    outs.append((out, flag, rows))
                (o0, f0, r0), (o1, f1, r1) = outs
                what = "B=%d batch %d/%d layers=%d" % (B, k, len(all_b), sum(x is not None for x in layers) + 1)
                assert torch.equal(f0, f1), what
                assert torch.equal(r0, r1), what
                assert torch.equal(o0, o1), what                               # batch rows equal, all others untouched
                want = S
                for t in layers:
                    if t is not None:
                        want = want + t
                want = want + Y
                sel = r1.long()
                assert torch.equal(o1[sel], want[sel]), what                   # the full product on the wanted rows
                assert int(f1.sum()) == len(torch.unique(sel)), what
        # the device planner's lists against the host statement of the planner
        stride = hop.stride
        sched = hop.buf[:hop.n_batches * stride * 16].cpu().numpy().view(np.int32).reshape(hop.n_batches, stride, 4)
        keys = keys_dev.cpu().numpy().view(np.uint64)
        for k in picks:
            kk = np.ascontiguousarray(keys[3 * k * B:3 * k * B + 3 * all_b[k][0].numel()])
            out = np.zeros((stride, 4), np.int32)
            n = host.wp_plan_batch(indptr.ctypes.data, N, kk.ctypes.data, len(kk), stride, out.ctypes.data, None, None)
            assert n >= 0
            assert out.tobytes() == np.ascontiguousarray(sched[k]).tobytes(), "B=%d batch %d: work list differs" % (B, k)


def test_planned_hop_equals_the_by_batch_hop_gowalla():
    A, train, U, I = _gowalla()
    _hop_case(A, train, U, I, batches=(1, 64, 1024, 4096), seed=1)


@pytest.mark.parametrize("seed", [3, 4])
def test_planned_hop_equals_the_by_batch_hop_random(seed):
    A, train, U, I = _random(seed)
    _hop_case(A, train, U, I, batches=(1, 2, 37, 512, 4096), seed=seed)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_fifty_steps_across_an_epoch_boundary_train_the_same_tables(L, monkeypatch):
    import torch
    from neurec_amd import engine as E
    from neurec_amd.trainer import BprEpochSampler, LightGCNEngine
    A, train, U, I = _random(11)
    B = 1024
    trc = E.DeviceCSR.from_scipy(train)
    n_batches = (train.nnz + B - 1) // B
    assert 2 <= n_batches < 50, n_batches                                     # 50 steps pass at least one epoch boundary
    E0 = np.random.RandomState(7).uniform(-0.05, 0.05, (U + I, 64)).astype(np.float32)
    tables = []
    for planned in ("0", "1"):
        monkeypatch.setenv("NEUREC_SPMM_WANTED_PLANNED", planned)
        lg = LightGCNEngine(A, U, I, E0, L, 0.01, 1e-3, B)
        assert lg._hop.ok == (planned == "1")
        sampler = BprEpochSampler(trc, I, batch_size=B, seed=2018, plan_users=U)
        loss2 = torch.zeros(2, device="cuda")
        steps, losses = 0, []
        while steps < 50:
            for b in sampler.batches():
                lg.step(b[0], b[1], b[2], loss2, plan=b.plan)
                losses.append(loss2.clone())
                steps += 1
                if steps == 50:
                    break
        assert sampler.epoch >= 2
        tables.append((lg.E0.clone(), lg.m.clone(), lg.v.clone(), torch.stack(losses)))
    for a, b in zip(*tables):
        assert torch.equal(a, b)
