"""The lane-group SpMM's non-zeros as 4-byte words (nrhip_spmm_blocked_pack_factored): word = column | code of the
column's factor, value = float32(row factor * table[code]), every product verified against the stored value when the
plan is packed.  The words are another encoding of the same matrix, so every case is compared BIT FOR BIT with the same
call on the two-array form (nrhip_spmm_blocked_tune_packed(0)):
  * a bipartite `pre` graph of 290 rows, split row set, with rows of 0, 1, 15, 16, 17, 63, 64, 65 and 130 non-zeros
    (the 16-entry chunk and the 64-entry segment) and a row of 230 (four segments);
  * d = 16, 32, 64; plain, addend, addend by flag, running sum; column-masked (the staged kernel, which keeps the
    two arrays and must not notice, and the general kernel, which reads the words, in a child process with
    NEUREC_SPMM_MASKED_FAST=0), row-masked, both masks; the ApplyAdam pass against the
    two-launch sequence; twenty LightGCN steps;
  * refusals leave the plan unpacked and the results unchanged: values that do not factor, 1,025 distinct factors
    (1,024 pack), a factor array that misses one value;
  * values_changed(): new values that do not factor are followed, the old ones pack again;
  * one product against float64, and canary rows behind Y in every equivalence case."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, I, EMPTY = 240, 40, 10
DEG = [230, 130, 65, 64, 63, 17, 16, 15, 1, 100] + [2 + (5 * j) % 40 for j in range(30)]
N = U + EMPTY + I
CANARY = 8            # rows behind Y that no kernel may touch


def _adjacency(adj_type="pre"):
    from neurec_amd.graph import lightgcn_adjacency
    assert len(DEG) == I
    rows = np.concatenate([(37 * j + np.arange(k)) % U for j, k in enumerate(DEG)])   # users U .. U+EMPTY-1: none
    cols = np.repeat(np.arange(I), DEG)
    return lightgcn_adjacency(rows, cols, U + EMPTY, I, adj_type)


@pytest.fixture(scope="module")
def case():
    import torch
    from neurec_amd import engine as E
    A = _adjacency()
    lens = np.diff(A.indptr)
    assert set([0, 1, 15, 16, 17, 63, 64, 65, 130]) <= set(lens.tolist()) and A.shape == (N, N)
    csr = E.SpmmCSR.from_scipy(A, split_row=U + EMPTY)
    for d in (16, 32, 64):
        assert csr.is_packed(d)
    rng = np.random.RandomState(5)
    X = torch.from_numpy(rng.randn(N, 64).astype(np.float32)).cuda()
    H = torch.from_numpy(rng.randn(N, 64).astype(np.float32)).cuda()
    S = torch.from_numpy(rng.randn(N, 64).astype(np.float32)).cuda()
    return csr, A, X, H, S


@pytest.fixture
def packed():
    """nrhip_spmm_blocked_tune_packed(on); the default is put back afterwards"""
    from neurec_amd import engine as E
    try:
        yield lambda on: E.call("nrhip_spmm_blocked_tune_packed", int(on))
    finally:
        E.call("nrhip_spmm_blocked_tune_packed", 1)


def _same(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _out(d, fill=7.0):
    """an output of N rows with canary rows behind it: (the view the kernel gets, the whole buffer)"""
    import torch
    whole = torch.full((N + CANARY, d), fill, device="cuda")
    whole[N:] = 12345.0
    return whole[:N], whole


def _canary_ok(whole):
    return bool((whole[N:] == 12345.0).all())


def _both(packed, run):
    """run() with the words and with the two arrays"""
    packed(1)
    a = run()
    packed(0)
    b = run()
    packed(1)
    return a, b


@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("form", ["plain", "addend", "addend_flag", "running_sum"])
def test_the_full_pass_on_words_equals_the_two_array_pass(case, packed, d, form):
    import torch
    csr, _, X, H, S = case
    Xd, Hd, Sd = (t[:, :d].contiguous() for t in (X, H, S))
    flags = (np.random.RandomState(9).rand(N) < 0.33).astype(np.uint8)
    fl = torch.from_numpy(flags).cuda()
    Hf = Hd * fl[:, None]

    def run():
        y, yw = _out(d)
        so, sow = _out(d)
        if form == "plain":
            csr.matmul(Xd, out=y)
        elif form == "addend":
            csr.matmul(Xd, out=y, addend=Hd)
        elif form == "addend_flag":
            csr.matmul(Xd, out=y, addend=Hf, addend_row_flag=fl)
        else:
            csr.matmul(Xd, out=y, addend=Hd, sum_in=Sd, sum_out=so)
        assert _canary_ok(yw) and _canary_ok(sow)
        return torch.cat([yw, sow])

    a, b = _both(packed, run)
    assert csr.is_packed(d) and _same(a, b)
    assert not _same(a[:N], torch.full_like(a[:N], 7.0))


def _masks():
    import torch
    rng = np.random.RandomState(21)
    col = (rng.rand(N) < 0.3).astype(np.uint8)
    row = (rng.rand(N) < 0.4).astype(np.uint8)
    col[U + EMPTY:U + EMPTY + 10] = 1                      # the long rows' columns among them
    row[U + EMPTY:U + EMPTY + 10] = 1
    return torch.from_numpy(col).cuda(), torch.from_numpy(row).cuda()


@pytest.mark.parametrize("masks", ["columns", "rows", "both"])
def test_the_masked_hops_on_words_equal_the_two_array_hops(case, packed, masks):
    import torch
    csr, _, X, H, S = case
    col, row = _masks()
    Xm = X * col[:, None]                                  # the promise of a column mask: the other rows are zero

    def run():
        y, yw = _out(64)
        so, sow = _out(64)
        kw = dict(x_row_nonzero=col) if masks == "columns" else dict(y_row_wanted=row) if masks == "rows" else \
            dict(x_row_nonzero=col, y_row_wanted=row)
        csr.matmul(Xm if masks != "rows" else X, out=y, addend=Xm if masks == "columns" else H, sum_in=S, sum_out=so,
                   **kw)
        assert _canary_ok(yw) and _canary_ok(sow)
        return torch.cat([yw, sow])

    a, b = _both(packed, run)
    assert _same(a, b)
    if masks == "columns":                                 # and the masked hop is the full product of the masked operand
        full, _ = _out(64)
        csr.matmul(Xm, out=full, addend=Xm)
        assert _same(a[:N], full)


_CHILD = r"""
import numpy as np, torch, sys
sys.path.insert(0, %r)
from tests.test_spmm_packed_gpu import _adjacency, _masks, N, U, EMPTY
from neurec_amd import engine as E
csr = E.SpmmCSR.from_scipy(_adjacency(), split_row=U + EMPTY)
assert csr.is_packed(64)
rng = np.random.RandomState(5)
X = torch.from_numpy(rng.randn(N, 64).astype(np.float32)).cuda()
col, row = _masks()
Xm = X * col[:, None]
outs = []
for on in (1, 0):
    E.call("nrhip_spmm_blocked_tune_packed", on)
    for kw in (dict(x_row_nonzero=col), dict(x_row_nonzero=col, y_row_wanted=row)):
        y = torch.full((N, 64), 7.0, device="cuda")
        csr.matmul(Xm, out=y, addend=Xm, **kw)
        outs.append(y)
full = torch.empty(N, 64, device="cuda")
csr.matmul(Xm, out=full, addend=Xm)
ok = torch.equal(outs[0].view(torch.int32), outs[2].view(torch.int32)) and \
    torch.equal(outs[1].view(torch.int32), outs[3].view(torch.int32)) and \
    torch.equal(outs[0].view(torch.int32), full.view(torch.int32))
print("GENERAL_MASKED_OK" if ok else "GENERAL_MASKED_DIFFERS")
"""


def test_the_general_masked_kernel_reads_words_too():
    """NEUREC_SPMM_MASKED_FAST=0 is read when a plan is created: a child process"""
    env = dict(os.environ, NEUREC_SPMM_MASKED_FAST="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "GENERAL_MASKED_OK" in r.stdout, r.stdout + r.stderr


def test_the_adam_pass_on_words(case, packed):
    import torch
    from neurec_amd import engine as E
    csr, _, X, H, _ = case
    rng = np.random.RandomState(17)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    Gb = dev(rng.randn(N, 64) * 0.01)
    var0, m0, v0 = rng.randn(N, 64), rng.randn(N, 64) * 0.01, rng.rand(N, 64) * 1e-3
    st = E.AdamState(0.01)
    st.advance()
    # two launches on the two arrays
    packed(0)
    var_a, m_a, v_a = dev(var0), dev(m0), dev(v0)
    Y = csr.matmul(X, out=torch.empty_like(X), addend=H)
    E.adam_dense2(var_a, m_a, v_a, Y, Gb, st)
    # one launch, on the words and on the two arrays
    for on in (1, 0):
        packed(on)
        var_b, m_b, v_b = dev(var0), dev(m0), dev(v0)
        assert csr.matmul_adam(X, H.clone(), Gb.clone(), var_b, m_b, v_b, st)
        for a, b in ((var_a, var_b), (m_a, m_b), (v_a, v_b)):
            assert _same(a, b)


def test_twenty_lightgcn_steps_train_the_same_tables(packed):
    import torch
    from neurec_amd.trainer import LightGCNEngine
    A = _adjacency()
    B = 48
    E0 = np.random.RandomState(7).uniform(-0.05, 0.05, (N, 64)).astype(np.float32)
    rng = np.random.RandomState(6)
    batches = [tuple(torch.from_numpy(x).cuda() for x in
                     (rng.randint(0, U, B).astype(np.int32), rng.randint(0, I, B).astype(np.int32),
                      rng.randint(0, I, B).astype(np.int32))) for _ in range(20)]
    tables = []
    for on in (1, 0):
        packed(on)
        lg = LightGCNEngine(A, U + EMPTY, I, E0, 3, 0.01, 1e-3, B)
        assert lg.A.is_packed(64)
        loss = torch.zeros(2, device="cuda")
        for u, p, n in batches:
            lg.step(u, p, n, loss)
        tables.append((lg.E0.clone(), lg.m.clone(), lg.v.clone(), loss.clone()))
    for a, b in zip(*tables):
        assert _same(a, b)
    assert not _same(tables[0][0], torch.from_numpy(E0).cuda())


def _same_as_unpacked(csr, packed, X):
    import torch
    a, b = _both(packed, lambda: csr.matmul(X, out=torch.empty_like(X)))
    return _same(a, b)


def test_values_that_do_not_factor_stay_on_the_two_arrays(case, packed):
    import torch
    from neurec_amd import engine as E
    _, _, X, _, _ = case
    csr = E.SpmmCSR.from_scipy(_adjacency("mean"), split_row=U + EMPTY)
    assert csr.ensure_schedule(64) and not csr.is_packed(64)
    assert _same_as_unpacked(csr, packed, X)


@pytest.mark.parametrize("n_factors", [1024, 1025])
def test_a_table_of_1024_factors_packs_and_1025_do_not(packed, n_factors):
    """row-constant values, one distinct value per row for n_factors - 1 rows (and the column factor 1.0, which is
    none of them): the table the kernels keep in LDS holds 1,024"""
    import scipy.sparse as sp
    import torch
    from neurec_amd import engine as E
    from neurec_amd.graph import factor_values
    n = 1100
    rng = np.random.RandomState(3)
    lens = 1 + (np.arange(n) % 3)
    rows = np.repeat(np.arange(n), lens)
    cols = np.concatenate([rng.choice(n, k, replace=False) for k in lens])
    per_row = 2.0 + (np.minimum(np.arange(n), n_factors - 2)).astype(np.float32) / 4096
    assert len(np.unique(np.append(per_row, np.float32(1)))) == n_factors
    m = sp.csr_matrix((per_row[rows].astype(np.float32), (rows, cols)), shape=(n, n))
    assert factor_values(m) is not None
    csr = E.SpmmCSR.from_scipy(m)
    assert csr.ensure_schedule(64)
    assert csr.is_packed(64) == (n_factors == 1024)
    X = torch.from_numpy(rng.randn(n, 64).astype(np.float32)).cuda()
    assert _same_as_unpacked(csr, packed, X)


def test_a_factor_array_that_misses_one_value_is_refused(case, packed):
    import torch
    from neurec_amd import engine as E
    from neurec_amd.graph import factor_values
    _, A, X, _, _ = case
    csr = E.SpmmCSR.from_scipy(A, split_row=U + EMPTY)
    assert csr.is_packed(64)
    want = csr.matmul(X, out=torch.empty_like(X))
    rf, cf = (f.copy() for f in factor_values(A))
    cf[U + EMPTY + 3] = np.nextafter(cf[U + EMPTY + 3], np.float32(1))          # one column's factor, 1 ulp off
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    took = C.c_int(-1)
    E.call("nrhip_spmm_blocked_pack_factored", csr.blocked, ptr(csr.indices), ptr(csr.vals),
           rf.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p), N, stream, C.byref(took))
    assert took.value == 0 and not csr.is_packed(64)
    assert _same(csr.matmul(X, out=torch.empty_like(X)), want)
    # the factors handed in directly, right: packed again, same bits
    rf, cf = factor_values(A)
    E.call("nrhip_spmm_blocked_pack_factored", csr.blocked, ptr(csr.indices), ptr(csr.vals),
           rf.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p), N, stream, C.byref(took))
    assert took.value == 1 and csr.is_packed(64)
    assert _same(csr.matmul(X, out=torch.empty_like(X)), want)


def test_values_changed_follows_the_values_and_packs_again(case, packed):
    import torch
    from neurec_amd import engine as E
    _, A, X, _, _ = case
    csr = E.SpmmCSR.from_scipy(A, split_row=U + EMPTY)
    assert csr.is_packed(64)
    want_pre = csr.matmul(X, out=torch.empty_like(X))
    old = csr.vals.clone()
    other = A.copy()
    other.data = (A.data * (1 + 0.25 * np.random.RandomState(4).rand(A.nnz))).astype(np.float32)
    csr.vals[:A.nnz] = torch.from_numpy(other.data).cuda()
    csr.values_changed()
    assert not csr.is_packed(64)
    fresh = E.SpmmCSR.from_scipy(other, split_row=U + EMPTY)
    got = csr.matmul(X, out=torch.empty_like(X))
    assert _same(got, fresh.matmul(X, out=torch.empty_like(X))) and not _same(got, want_pre)
    csr.vals.copy_(old)
    csr.values_changed()
    assert csr.is_packed(64)
    assert _same(csr.matmul(X, out=torch.empty_like(X)), want_pre)


def test_the_packed_product_against_float64(case):
    """a row is an ordered float32 sum of n <= 230 rounded products: |error| <= (n + 1) * 2^-24 * sum |a| |x|
    (one rounding per product, one per addition, first order), taken per element with n = 231"""
    import torch
    csr, A, X, _, _ = case
    assert csr.is_packed(64)
    got = csr.matmul(X, out=torch.empty_like(X)).cpu().numpy().astype(np.float64)
    x64 = X.cpu().numpy().astype(np.float64)
    a64 = A.astype(np.float64)
    ref = a64 @ x64
    bound = 231 * 2.0 ** -24 * (abs(a64) @ np.abs(x64)) * 1.01 + 1e-30
    print("largest error / bound: %.3f" % float(np.max(np.abs(got - ref) / bound)))
    assert np.all(np.abs(got - ref) <= bound)
