"""WRMF (implicit ALS) on the HIP engine: the two half-sweeps of WRMF.py:66-84 as batched on-device solves.

The reference updates one row per `sess.run` (WRMF.py:47-59: a dense [I, d] product against a column of the U x I
matrices Cui / Pui, then tf.linalg.solve and scatter_update).  Inside a half-sweep every row reads only the other
table, so the per-row loop is one batched solve over all rows of that side: the users against the current items,
then the items against the users just written.  Each half is a Gram launch (G = Y^T Y) and a solve launch
(csrc/wrmf.hip); the train matrix enters only as its sparsity pattern, in CSR form on both sides.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import torch

from ._lib import call
from .engine import Workspace, _ptr, _stream, require_gpu


class _Side:
    """one side's CSR (rows = the side solved, columns = the other side) + its chunk plan, on the device"""

    def __init__(self, mat, dev):
        m = sp.csr_matrix(mat, copy=True)
        m.sum_duplicates()
        m.sort_indices()
        h_indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
        self.n_rows, self.n_cols = m.shape
        self.nnz = int(h_indptr[-1])
        self.indptr = torch.from_numpy(h_indptr).to(dev)
        idx = np.ascontiguousarray(m.indices, dtype=np.int32)
        self.indices = torch.from_numpy(idx if len(idx) else np.zeros(1, np.int32)).to(dev)
        n = C.c_int(0)
        call("nrhip_wrmf_chunk_plan", h_indptr.ctypes.data_as(C.c_void_p), self.n_rows, None, None, C.byref(n))
        row_chunk = np.empty(max(self.n_rows, 1), np.int32)
        chunk_row = np.empty(max(n.value, 1), np.int32)
        call("nrhip_wrmf_chunk_plan", h_indptr.ctypes.data_as(C.c_void_p), self.n_rows,
             row_chunk.ctypes.data_as(C.c_void_p), chunk_row.ctypes.data_as(C.c_void_p), C.byref(n))
        self.n_chunks = n.value
        self.row_chunk = torch.from_numpy(row_chunk).to(dev)
        self.chunk_row = torch.from_numpy(chunk_row).to(dev)


class WRMFEngine:
    """P [U, d] and Q [I, d] on the device, trained by `epoch()` (users, then items).

    `train` is the U x I train matrix (any scipy sparse form; only its pattern is read).  `alpha` is the confidence
    weight (Cui = alpha on stored entries), `reg` the ridge lambda (reg_mf), which must be > 0.  The initial user
    table only fixes the shape: the first half-sweep overwrites every row of it."""

    def __init__(self, P0, Q0, train, alpha, reg):
        if not reg > 0:
            raise ValueError("WRMF needs reg_mf > 0 (the solves use a Cholesky factorisation of "
                             "Y^T Y + alpha Y^T C Y + reg_mf I), got %r" % (reg,))
        if not alpha >= 0:
            raise ValueError("WRMF needs alpha >= 0, got %r" % (alpha,))
        dev = require_gpu()
        P0, Q0 = np.asarray(P0, np.float32), np.asarray(Q0, np.float32)
        U, I = train.shape
        if P0.shape[0] != U or Q0.shape[0] != I or P0.shape[1] != Q0.shape[1]:
            raise ValueError("table shapes %s / %s do not fit a %d x %d train matrix" % (P0.shape, Q0.shape, U, I))
        self.d = int(P0.shape[1])
        self.alpha, self.reg = float(alpha), float(reg)
        nbytes = C.c_size_t(0)
        train = sp.csr_matrix(train)
        self.users = _Side(train, dev)                 # rows u, columns = items of u
        self.items = _Side(train.T.tocsr(), dev)       # rows i, columns = users of i
        call("nrhip_wrmf_workspace_bytes", self.d, max(self.users.n_chunks, self.items.n_chunks), C.byref(nbytes))
        self.P = torch.from_numpy(np.ascontiguousarray(P0)).to(dev)
        self.Q = torch.from_numpy(np.ascontiguousarray(Q0)).to(dev)
        self.G = torch.zeros((self.d, self.d), dtype=torch.float32, device=dev)
        self._ws = Workspace()
        self._ws_bytes = int(nbytes.value)

    def _half(self, side, Y, X):
        """X = the solves of `side`'s rows against Y (one Gram launch + one solve launch, no host sync)"""
        ws = self._ws.get(self._ws_bytes)
        st = _stream()
        call("nrhip_wrmf_gram", _ptr(Y, torch.float32), Y.shape[0], self.d, _ptr(self.G), _ptr(ws),
             self._ws_bytes, st)
        call("nrhip_wrmf_solve", _ptr(side.indptr), _ptr(side.indices), side.n_rows, _ptr(Y, torch.float32),
             Y.shape[0], _ptr(self.G), self.d, C.c_float(self.alpha), C.c_float(self.reg), _ptr(side.row_chunk),
             _ptr(side.chunk_row), side.n_chunks, _ptr(X, torch.float32), _ptr(ws), self._ws_bytes, st)

    def solve_users(self):
        self._half(self.users, self.Q, self.P)

    def solve_items(self):
        self._half(self.items, self.P, self.Q)

    def epoch(self):
        """WRMF.py:69-80: every user against the current items, then every item against the new users"""
        self.solve_users()
        self.solve_items()

    def tables(self):
        return self.P, self.Q
