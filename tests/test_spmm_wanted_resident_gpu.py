"""Store policies of the SpMM row outputs in a LightGCN step: the column-masked backward hop writes Y plainly,
nontemporally or through (nrhip_spmm_blocked_tune_store), and the d = 64 full passes write Y through.  A policy is a
cache hint and may not change a bit:
  * a hand-made bipartite graph of 600 rows with every kind of row (a hub of 540 non-zeros, rows of 65 .. 512 in
    every segment count class, rows of exactly 64 and 65, many short rows) and a batch (B = 48) that holds them all;
  * the column-masked hop's Y under the three policies identical to the plain one's and to the full product;
  * twenty steps of LightGCNEngine.step under the shipped policy against step_reference with plain stores in its
    masked hop: losses, E0, m, v identical.
(The file is named after the resident-round form of the batch-rows forward hop, which did not pay and is not in the tree:
profiles/r18_latency_chain.txt.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U, I, D, B = 560, 40, 64, 48
# users of item j: a window of DEG[j] consecutive users (mod U) that starts at 37 j
HUB = 540                                                   # 9 segments: two chunks, 16 slots
DEG = [HUB, 300, 400,                                       # 8 slots each
       130, 200, 250, 256,                                  # 4 slots each
       65, 100, 128, 70, 80, 90, 110, 120,                  # 2 slots each
       64] + [3 + (5 * j) % 40 for j in range(24)]          # exactly 64; short rows
N_BIG = 16                                                  # items 0 .. 15 are the ones above


def _graph():
    import scipy.sparse as sp
    from neurec_amd.graph import lightgcn_adjacency
    assert len(DEG) == I
    rows = np.concatenate([(37 * j + np.arange(k)) % U for j, k in enumerate(DEG)])
    cols = np.repeat(np.arange(I), DEG)
    train = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(U, I))
    assert train.nnz == len(rows) and np.diff(train.indptr).min() >= 1
    assert np.array_equal(np.diff(train.tocsc().indptr), DEG)
    return lightgcn_adjacency(rows, cols, U, I, "pre"), train


def _batch(rng):
    """48 triplets whose rows hold every big item, the row of 64 and short rows of both kinds, some of them twice"""
    users = rng.choice(U, B, replace=False).astype(np.int32)
    pos = np.concatenate([np.arange(N_BIG), rng.randint(N_BIG, I, B - N_BIG)]).astype(np.int32)
    neg = rng.randint(N_BIG, I, B).astype(np.int32)
    return users, pos, neg


def _stream(n_batches, seed):
    """a stream of n_batches batches (the first one is _batch), planned the way the sampler plans an epoch"""
    import torch
    from neurec_amd import engine as E
    from neurec_amd.trainer import TripletBatch
    rng = np.random.RandomState(seed)
    u, p, n = _batch(rng)
    for _ in range(n_batches - 1):
        u = np.concatenate([u, rng.randint(0, U, B).astype(np.int32)])
        p = np.concatenate([p, rng.randint(0, I, B).astype(np.int32)])
        n = np.concatenate([n, rng.randint(0, I, B).astype(np.int32)])
    u, p, n = (torch.from_numpy(x).cuda() for x in (u, p, n))
    plans = E.bpr_plan(u, p, n, B, U)
    out = []
    for k in range(n_batches):
        plan = plans[3 * k * B:3 * (k + 1) * B]
        plan.epoch_plans, plan.batch_index = (plans, B, 1), k
        out.append(TripletBatch(u[k * B:(k + 1) * B], p[k * B:(k + 1) * B], n[k * B:(k + 1) * B], plan))
    return out


@pytest.fixture
def tune():
    """nrhip_spmm_blocked_tune_store(policy); the default is put back afterwards"""
    from neurec_amd import engine as E
    try:
        yield lambda store: E.call("nrhip_spmm_blocked_tune_store", int(store))
    finally:
        E.call("nrhip_spmm_blocked_tune_store", -1)


def test_twenty_steps_train_the_tables_of_the_reference_sequence_with_plain_stores(tune):
    import torch
    from neurec_amd.trainer import LightGCNEngine
    A, _ = _graph()
    E0 = np.random.RandomState(7).uniform(-0.05, 0.05, (U + I, D)).astype(np.float32)
    a, b = LightGCNEngine(A, U, I, E0, 3, 0.01, 1e-3, B), LightGCNEngine(A, U, I, E0, 3, 0.01, 1e-3, B)
    assert a._hop.ok
    la, lb = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    for batch in _stream(20, seed=6):
        tune(-1)                                             # the step: the shipped store policy
        a.step(batch[0], batch[1], batch[2], la, plan=batch.plan)
        tune(0)                                              # the spelled-out sequence: plain stores
        b.step_reference(batch[0], batch[1], batch[2], lb, plan=batch.plan)
        assert torch.equal(la, lb)
    for x, y in ((a.E0, b.E0), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(x, y)


def test_the_column_masked_hop_stores_the_same_bytes_under_every_policy(tune):
    import torch
    from neurec_amd import engine as E
    A, _ = _graph()
    N = U + I
    csr = E.SpmmCSR.from_scipy(A, split_row=U)
    assert csr.ensure_schedule(D)
    bu, bp, bn = _stream(1, seed=5)[0]
    flag = torch.zeros(N, dtype=torch.uint8, device="cuda")
    flag[torch.cat([bu, bp + U, bn + U]).long()] = 1
    g = torch.Generator(device="cuda")
    g.manual_seed(10)
    H = torch.randn(N, D, generator=g, device="cuda") * flag[:, None]        # zero off the batch rows, as in the step
    outs = []
    for store in (0, 1, 2):
        tune(store)
        Y = torch.full((N, D), 3.0, device="cuda")
        csr.matmul(H, out=Y, addend=H, x_row_nonzero=flag)
        outs.append(Y)
    full = torch.empty(N, D, device="cuda")
    csr.matmul(H, out=full, addend=H)
    assert torch.equal(outs[0], full)
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
