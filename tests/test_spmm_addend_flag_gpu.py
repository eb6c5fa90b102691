"""The lane-group full pass with a row-sparse addend read by flag (nrhip_spmm_csr_flagged; the inner backward hops of
a LightGCN step hand it H and the batch's row flags), and the same flags staged for the ApplyAdam epilogue.  The flags
are a promise (flag 0 = the addend row is all zero), so every case is compared bit for bit with the dense-addend
product of the same matrix:
  * a bipartite graph of 610 rows with every kind of row the pass distinguishes (no non-zeros, 1, 15, 16, 17, 64, 65,
    a hub of 540 = nine segments, rows of 2 .. 8 segments) — more rows than one workgroup's list on any device;
  * no row flagged, all rows flagged, a random third flagged;
  * every row flagged ALONE, one launch per row, all other addend rows NaN: a workgroup's row list is the planner's
    business (dealt by cost, per device), so instead of reading it the sweep puts the one flagged row at every position
    of every list, the first and the last included, and a single NaN read from an unflagged row fails the case;
  * the running-sum form (sum_in / sum_out), a narrower width (the kernel is one template), and at d = 16 row lists
    longer than a workgroup has threads;
  * the flags ignored process-wide (nrhip_spmm_blocked_tune_addend_flag(0)) give the same bits;
  * the ApplyAdam pass with NaN in the unflagged rows of addend and grad_b against the two-pass sequence on zeros, with
    the consumed rows and the flags re-armed."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U, I, EMPTY = 560, 40, 10
DEG = [540, 300, 400, 130, 200, 250, 256, 65, 100, 128, 70, 80, 90, 110, 120, 64,
       1, 15, 16, 17] + [3 + (5 * j) % 40 for j in range(20)]
N = U + EMPTY + I


@pytest.fixture(scope="module")
def case():
    """the matrix on the device at d = 64, an operand, a dense addend, and the dense-addend product (computed once)"""
    import torch
    from neurec_amd import engine as E
    from neurec_amd.graph import lightgcn_adjacency
    assert len(DEG) == I
    rows = np.concatenate([(37 * j + np.arange(k)) % U for j, k in enumerate(DEG)])   # users U .. U+EMPTY-1: none
    cols = np.repeat(np.arange(I), DEG)
    A = lightgcn_adjacency(rows, cols, U + EMPTY, I, "pre")
    lens = np.diff(A.tocsr().indptr)
    assert set([0, 1, 15, 16, 17, 64, 65, 540]) <= set(lens.tolist()) and A.shape == (N, N)
    csr = E.SpmmCSR.from_scipy(A, split_row=U + EMPTY)
    assert csr.ensure_schedule(64)
    rng = np.random.RandomState(5)
    X = torch.from_numpy(rng.randn(N, 64).astype(np.float32)).cuda()
    H = torch.from_numpy(rng.randn(N, 64).astype(np.float32)).cuda()
    return csr, X, H, rng


def _masked_addend(H, flags, fill):
    """H on the flagged rows, `fill` (0 or NaN) on the others"""
    import torch
    keep = torch.from_numpy(flags.astype(bool)).cuda()[:, None]
    return torch.where(keep, H, torch.full_like(H, fill))


def _same(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("which", ["none", "all", "third"])
def test_flagged_addend_equals_the_dense_addend(case, which):
    import torch
    csr, X, H, rng = case
    flags = {"none": np.zeros(N, np.uint8), "all": np.ones(N, np.uint8),
             "third": (np.random.RandomState(9).rand(N) < 0.33).astype(np.uint8)}[which]
    want = csr.matmul(X, out=torch.empty_like(X), addend=_masked_addend(H, flags, 0.0))
    got = csr.matmul(X, out=torch.full_like(X, 7.0), addend=_masked_addend(H, flags, float("nan")),
                     addend_row_flag=torch.from_numpy(flags).cuda())
    assert not torch.isnan(got).any() and _same(got, want)
    # the running-sum form: Y and sum_out both
    S = torch.from_numpy(np.random.RandomState(3).randn(N, 64).astype(np.float32)).cuda()
    so_a, so_b = torch.empty_like(X), torch.empty_like(X)
    csr.matmul(X, out=torch.empty_like(X), addend=_masked_addend(H, flags, 0.0), sum_in=S, sum_out=so_a)
    csr.matmul(X, out=torch.empty_like(X), addend=_masked_addend(H, flags, float("nan")), sum_in=S, sum_out=so_b,
               addend_row_flag=torch.from_numpy(flags).cuda())
    assert _same(so_a, so_b)


def test_every_row_flagged_alone_reads_that_addend_row_only(case):
    import torch
    csr, X, H, _ = case
    # dense reads; a row's result depends on its own addend row only: y + 0 on an unflagged row, y + H[r] on the flagged
    base = csr.matmul(X, out=torch.empty_like(X), addend=torch.zeros_like(H))
    dense_all = csr.matmul(X, out=torch.empty_like(X), addend=H)
    nan = torch.full_like(H, float("nan"))
    flags = torch.zeros(N, dtype=torch.uint8, device="cuda")
    got = torch.empty_like(X)
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    for r in range(N):
        flags.zero_()
        flags[r] = 1
        addend = nan.clone()
        addend[r] = H[r]
        csr.matmul(X, out=got, addend=addend, addend_row_flag=flags)
        want = base.clone()
        want[r] = dense_all[r]
        bad += (got.view(torch.int32) != want.view(torch.int32)).any().long()
    assert int(bad) == 0


def test_the_flags_can_be_ignored_process_wide(case):
    import torch
    from neurec_amd import engine as E
    csr, X, H, _ = case
    flags = (np.random.RandomState(11).rand(N) < 0.2).astype(np.uint8)
    Hs = _masked_addend(H, flags, 0.0)
    fl = torch.from_numpy(flags).cuda()
    on = csr.matmul(X, out=torch.empty_like(X), addend=Hs, addend_row_flag=fl)
    try:
        E.call("nrhip_spmm_blocked_tune_addend_flag", 0)
        off = csr.matmul(X, out=torch.empty_like(X), addend=Hs, addend_row_flag=fl)
    finally:
        E.call("nrhip_spmm_blocked_tune_addend_flag", 1)
    assert _same(on, off)


def test_flags_need_an_addend_and_no_masks(case):
    import torch
    csr, X, H, _ = case
    fl = torch.ones(N, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        csr.matmul(X, out=torch.empty_like(X), addend_row_flag=fl)
    with pytest.raises(ValueError):
        csr.matmul(X, out=torch.empty_like(X), addend=H, addend_row_flag=fl, x_row_nonzero=fl)


def test_a_narrower_width_takes_the_flags_too(case):
    import torch
    csr, X, H, _ = case
    assert csr.ensure_schedule(32)
    X32, H32 = X[:, :32].contiguous(), H[:, :32].contiguous()
    flags = (np.random.RandomState(13).rand(N) < 0.5).astype(np.uint8)
    want = csr.matmul(X32, out=torch.empty_like(X32), addend=_masked_addend(H32, flags, 0.0))
    got = csr.matmul(X32, out=torch.empty_like(X32), addend=_masked_addend(H32, flags, float("nan")),
                     addend_row_flag=torch.from_numpy(flags).cuda())
    assert _same(got, want)
    csr.ensure_schedule(64)


def test_a_row_list_longer_than_the_workgroup_has_threads():
    """d = 16 keeps up to 1,664 row accumulators per workgroup: 12,000 rows on 8 workgroups give every one a list of
    ~1,500 rows, so the staging loop of the prologue takes a second turn for some threads"""
    import torch
    from neurec_amd import engine as E
    from neurec_amd.graph import lightgcn_adjacency
    rng = np.random.RandomState(23)
    nu, ni, d = 11000, 1000, 16
    n = nu + ni
    A = lightgcn_adjacency(np.repeat(np.arange(nu), 2), rng.randint(0, ni, 2 * nu), nu, ni, "pre")
    csr = E.SpmmCSR.from_scipy(A)
    nbytes = C.c_size_t(0)
    E.call("nrhip_spmm_blocked_plan_bytes", n, csr.nnz, d, C.byref(nbytes))
    buf = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    plan = C.c_void_p(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    E.call("nrhip_spmm_blocked_plan_create", csr.h_indptr.ctypes.data_as(C.c_void_p),
           csr.h_indices.ctypes.data_as(C.c_void_p), n, 0, d, 0, 8, 0, 0, 0, 0, ptr(buf), buf.numel(), stream,
           C.byref(plan))
    try:
        nwg = C.c_int(0)
        E.call("nrhip_spmm_blocked_plan_info", plan, C.byref(nwg), None, None, None)
        assert nwg.value == 8 and n / 8 > 1024
        X = torch.from_numpy(rng.randn(n, d).astype(np.float32)).cuda()
        H = torch.from_numpy(rng.randn(n, d).astype(np.float32)).cuda()
        flags = (rng.rand(n) < 0.3).astype(np.uint8)
        fl = torch.from_numpy(flags).cuda()
        want, got = torch.empty_like(X), torch.empty_like(X)
        for out, addend, f in ((want, _masked_addend(H, flags, 0.0), None), (got, _masked_addend(H, flags, float("nan")), fl)):
            E.call("nrhip_spmm_blocked_flagged", plan, ptr(csr.indices), ptr(csr.vals), ptr(X), ptr(out), ptr(addend),
                   ptr(f) if f is not None else None, None, None, None, None, stream)
        assert _same(got, want)
    finally:
        E.call("nrhip_spmm_blocked_plan_destroy", plan)


def test_the_adam_pass_reads_flagged_rows_only_and_re_arms_them(case):
    import torch
    from neurec_amd import engine as E
    csr, X, H, _ = case
    rng = np.random.RandomState(17)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    Gb = dev(rng.randn(N, 64) * 0.01)
    var0, m0, v0 = rng.randn(N, 64), rng.randn(N, 64) * 0.01, rng.rand(N, 64) * 1e-3
    flags = np.zeros(N, np.uint8)
    flags[rng.choice(N, 150, replace=False)] = 1
    flags[[0, N - 1]] = 1
    st = E.AdamState(0.01)
    st.advance()
    # two passes on zero-filled sparse inputs
    var_a, m_a, v_a = dev(var0), dev(m0), dev(v0)
    Y = csr.matmul(X, out=torch.empty_like(X), addend=_masked_addend(H, flags, 0.0))
    E.adam_dense2(var_a, m_a, v_a, Y, _masked_addend(Gb, flags, 0.0), st)
    # one pass, NaN where the flags promise zero
    var_b, m_b, v_b = dev(var0), dev(m0), dev(v0)
    Hn, Gn, fl = _masked_addend(H, flags, float("nan")), _masked_addend(Gb, flags, float("nan")), \
        torch.from_numpy(flags).cuda()
    assert csr.matmul_adam(X, Hn, Gn, var_b, m_b, v_b, st, row_flag=fl)
    for a, b in ((var_a, var_b), (m_a, m_b), (v_a, v_b)):
        assert _same(a, b)
    keep = torch.from_numpy(flags.astype(bool)).cuda()
    assert not fl.any() and not Hn[keep].any() and not Gn[keep].any()           # consumed rows and flags re-armed
    assert torch.isnan(Hn[~keep]).all() and torch.isnan(Gn[~keep]).all()        # the others were never touched
