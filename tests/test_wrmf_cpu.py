"""WRMF without a GPU: the C ABI surface of the new entries, the host-side chunk plan, and the golden trace of the
reference's own WRMF class (tests/golden/tfgraph_wrmf.npz) against the closed form the kernels implement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["nrhip_wrmf_chunk_plan", "nrhip_wrmf_workspace_bytes", "nrhip_wrmf_gram", "nrhip_wrmf_solve"]


def als_half(R, Y, alpha, lam):
    """one half-sweep in fp64: x_u = (Y^T Y + alpha sum_{j in N(u)} y_j y_j^T + lam I)^{-1} (1 + alpha) sum y_j"""
    Y = np.asarray(Y, np.float64)
    d = Y.shape[1]
    G = Y.T @ Y
    X = np.zeros((R.shape[0], d))
    for u in range(R.shape[0]):
        nb = R.indices[R.indptr[u]:R.indptr[u + 1]]
        if len(nb) == 0:
            continue
        Yn = Y[nb]
        X[u] = np.linalg.solve(G + alpha * Yn.T @ Yn + lam * np.eye(d), (1 + alpha) * Yn.sum(axis=0))
    return X


def als_epochs(R, Q0, alpha, lam, epochs):
    R = sp.csr_matrix(R)
    Rt = R.T.tocsr()
    Q, out = np.asarray(Q0, np.float64), []
    for _ in range(epochs):
        P = als_half(R, Q, alpha, lam)
        Q = als_half(Rt, P, alpha, lam)
        out.append((P, Q))
    return out


def test_header_declares_and_binding_covers_the_wrmf_entries():
    with open(os.path.join(ROOT, "include", "neurec_hip.h")) as f:
        text = f.read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, text), name
    assert "#define NRHIP_WRMF_CHUNK" in text and "WRMF.py:47-59" in text
    from neurec_amd import _lib
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)


def test_chunk_plan_and_workspace_query():
    """host code of the library: rows longer than the chunk get consecutive chunk ids in row order; widths above
    128 are refused as unsupported, 0 as an argument error"""
    from neurec_amd import _lib
    chunk = 1024
    deg = np.array([0, 5, chunk, chunk + 1, 3 * chunk, 7, 2 * chunk + 5], np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    n = C.c_int(-1)
    _lib.call("nrhip_wrmf_chunk_plan", indptr.ctypes.data_as(C.c_void_p), len(deg), None, None, C.byref(n))
    assert n.value == 2 + 3 + 3
    row_chunk = np.empty(len(deg), np.int32)
    chunk_row = np.empty(n.value, np.int32)
    _lib.call("nrhip_wrmf_chunk_plan", indptr.ctypes.data_as(C.c_void_p), len(deg),
              row_chunk.ctypes.data_as(C.c_void_p), chunk_row.ctypes.data_as(C.c_void_p), C.byref(n))
    assert row_chunk.tolist() == [-1, -1, -1, 0, 2, -1, 5]
    assert chunk_row.tolist() == [3, 3, 4, 4, 4, 6, 6, 6]
    sizes = []
    for d, nc in ((1, 0), (16, 0), (64, 8), (128, 8), (128, 100000)):
        b = C.c_size_t(0)
        _lib.call("nrhip_wrmf_workspace_bytes", d, nc, C.byref(b))
        sizes.append(b.value)
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert sizes[-1] >= 100000 * (128 * 128 + 128) * 4
    with pytest.raises(NotImplementedError, match="128"):
        _lib.call("nrhip_wrmf_workspace_bytes", 129, 0, C.byref(C.c_size_t(0)))
    with pytest.raises(ValueError):
        _lib.call("nrhip_wrmf_workspace_bytes", 0, 0, C.byref(C.c_size_t(0)))


def test_reference_trace_is_the_closed_form_als():
    """The fp64 tables the reference's WRMF class produced (LU solves, one row per sess.run, Cui / Pui dense) equal a
    batched fp64 ALS of the documented formula from the same Q0 — so the pattern alone counts, the initial user
    table does not, and rows without neighbours become exactly 0."""
    g = load_golden("tfgraph_wrmf")
    U, I = g["shape"]
    R = sp.csr_matrix((np.ones(len(g["indices"])), g["indices"], g["indptr"]), shape=(U, I))
    want = als_epochs(R, g["Q0"], float(g["alpha"]), float(g["reg_mf"]), int(g["epochs"]))
    for e, (P, Q) in enumerate(want):
        assert np.abs(g["f64_P"][e] - P).max() <= 1e-10 * max(1.0, np.abs(P).max())
        assert np.abs(g["f64_Q"][e] - Q).max() <= 1e-10 * max(1.0, np.abs(Q).max())
    deg_u, deg_i = np.diff(R.indptr), np.diff(R.tocsc().indptr)
    assert (deg_u == 0).any() and (deg_i == 0).any()
    assert np.all(g["f64_P"][:, deg_u == 0] == 0) and np.all(g["f64_Q"][:, deg_i == 0] == 0)
    # the evaluation saw P Q^T of the tables of that epoch
    users = g["ratings_users"]
    for e in range(int(g["epochs"])):
        S = g["f64_P"][e][users] @ g["f64_Q"][e].T
        assert np.abs(g["f64_ratings"][e] - S).max() <= 1e-12 * max(1.0, np.abs(S).max())
    assert [ln.split()[1] for ln in g["f32_log_lines"]] == ["1", "2"]
