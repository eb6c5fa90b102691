"""ItemKNN on the HIP engine: the item-item similarity of ItemKNN.py:60-214 / 395-547, cut to each column's top-K, and
the scores `train_matrix.dot(W_sparse)` of ItemKNN.py:573 for a batch of users — both on the device (csrc/itemknn.hip).

The reference forms a dense I x 100 product per block in numpy, loops over every column in Python and materialises the
dense U x I `ratings` matrix.  Here the host only prepares the O(nnz) value arrays in float64 (the mean-centring of
`adjusted` / `pearson`, the binarisation of the jaccard family, the per-item sums of squares and their powers — so the
means are exactly the reference's) and rounds them once; the Gram walk, the elementwise formula, the per-column
selection, the transpose of W and the scoring are kernels.

Tie rule: the larger value wins, among equal values the lower item index (the reference's order among equal values is
whatever `argpartition` leaves).  Euclidean: a pair with an item that has no interactions scores 0 and is never stored
(the reference: 0, or NaN for two such items).
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import torch

from ._lib import call
from .engine import Workspace, _ptr, _stream, require_gpu

MAX_NEIGHBOR = 1024           # NRHIP_ITEMKNN_MAX_NEIGHBOR
LDS_ITEMS = 12288             # NRHIP_ITEMKNN_LDS_ITEMS
_SLAB_FLOATS = 1 << 26        # default size of the [block][I] accumulator slab past LDS_ITEMS: 256 MiB

_KIND = {"cosine": 0, "adjusted": 0, "pearson": 0, "asymmetric": 0, "jaccard": 1, "tanimoto": 1, "dice": 2,
         "tversky": 3, "euclidean": 4}


def _dev(a, dtype, dev):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype)).to(dev)


def similarity_inputs(train, similarity, asymmetric_alpha=0.5):
    """(M, v, na, nb), all float64: the train CSR (sorted, duplicates summed), the value array the similarity works on
    (in M's CSR order) and the two per-item arrays of nrhip_itemknn_build — ItemKNN.py:319-393, 425-433, 89-90."""
    if similarity not in _KIND:
        raise ValueError("Cosine_Similarity: value for parameter 'mode' not recognized."
                         " Allowed values are: 'cosine', 'pearson', 'adjusted', 'asymmetric', 'jaccard', 'tanimoto',"
                         "dice, tversky."
                         " Passed value was '{}'".format(similarity))
    M = sp.csr_matrix(train, dtype=np.float64, copy=True)
    M.sum_duplicates()
    M.sort_indices()
    v = M.data.copy()
    if similarity == "adjusted":                # minus the mean of the row's stored entries
        per_row = np.diff(M.indptr)
        sums = np.asarray(M.sum(axis=1)).ravel()
        mean = np.zeros_like(sums)
        mean[per_row > 0] = sums[per_row > 0] / per_row[per_row > 0]
        v -= np.repeat(mean, per_row)
    elif similarity == "pearson":               # minus the mean of the column's stored entries
        per_col = np.bincount(M.indices, minlength=M.shape[1])
        sums = np.asarray(M.sum(axis=0)).ravel()
        mean = np.zeros_like(sums)
        mean[per_col > 0] = sums[per_col > 0] / per_col[per_col > 0]
        v -= mean[M.indices]
    elif _KIND[similarity] in (1, 2, 3):
        v[:] = 1.0
    ssq = np.asarray(sp.csr_matrix((v, M.indices, M.indptr), shape=M.shape).power(2).sum(axis=0)).ravel()
    if _KIND[similarity] in (1, 2, 3):
        na = nb = ssq
    elif similarity == "euclidean":
        na, nb = ssq, np.sqrt(ssq)
    elif similarity == "asymmetric":
        s = np.sqrt(ssq)
        na, nb = np.power(s, 2 * asymmetric_alpha), np.power(s, 2 * (1 - asymmetric_alpha))
    else:
        na = nb = np.sqrt(ssq)
    return M, v, na, nb


class ItemKNNEngine:
    """W (top-`neighbor` of every column of the item similarity) built at construction; `score(users)` -> [B, I].

    `train` is the U x I train matrix with its ratings (any scipy sparse form).  `block_cols` sets how many columns one
    launch of the build takes (default: all of them while the accumulator column fits LDS, else a 256 MiB slab)."""

    def __init__(self, train, neighbor, shrink=0, similarity="cosine", asymmetric_alpha=0.5, tversky_alpha=1.0,
                 tversky_beta=1.0, block_cols=None):
        M, v, na, nb = similarity_inputs(train, similarity, asymmetric_alpha)
        if int(neighbor) != neighbor or neighbor < 1:
            raise ValueError("ItemKNN needs neighbor >= 1, got %r" % (neighbor,))
        if neighbor > MAX_NEIGHBOR:
            raise NotImplementedError("ItemKNN: neighbor=%d is not supported (at most %d neighbours per item)"
                                      % (neighbor, MAX_NEIGHBOR))
        if not shrink >= 0:
            raise ValueError("ItemKNN needs shrink >= 0, got %r" % (shrink,))
        dev = require_gpu()
        self.similarity_name = similarity
        self.neighbor = int(neighbor)
        self.n_users, self.n_items = U, I = M.shape
        if block_cols is None:
            block_cols = I if I <= LDS_ITEMS else max(1, min(I, _SLAB_FLOATS // I))
        self.block_cols = int(block_cols)
        nbytes = C.c_size_t(0)
        call("nrhip_itemknn_workspace_bytes", I, self.neighbor, self.block_cols, C.byref(nbytes))
        # the pattern twice (CSR, CSC) with the similarity's values, and the raw ratings for the scoring
        sim_csc = sp.csr_matrix((v, M.indices, M.indptr), shape=M.shape).tocsc()
        sim_csc.sort_indices()
        self.indptr = _dev(M.indptr, np.int64, dev)
        self.indices = _dev(M.indices, np.int32, dev)
        self.ratings = _dev(M.data, np.float32, dev)
        sim_vals = _dev(v, np.float32, dev)
        csc_indptr = _dev(sim_csc.indptr, np.int64, dev)
        csc_users = _dev(sim_csc.indices, np.int32, dev)
        csc_vals = _dev(sim_csc.data, np.float32, dev)
        d_na, d_nb = _dev(na, np.float32, dev), _dev(nb, np.float32, dev)
        K = self.neighbor
        self.w_idx = torch.empty((I, K), dtype=torch.int32, device=dev)
        self.w_val = torch.empty((I, K), dtype=torch.float32, device=dev)
        self.w_cnt = torch.empty(I, dtype=torch.int32, device=dev)
        self.t_indptr = torch.zeros(I + 1, dtype=torch.int64, device=dev)
        self.t_cols = torch.zeros(I * K, dtype=torch.int32, device=dev)
        self.t_vals = torch.zeros(I * K, dtype=torch.float32, device=dev)
        ws = Workspace().get(nbytes.value)
        call("nrhip_itemknn_build", _ptr(csc_indptr), _ptr(csc_users), _ptr(csc_vals), _ptr(self.indptr),
             _ptr(self.indices), _ptr(sim_vals), _ptr(d_na), _ptr(d_nb), U, I, _KIND[similarity],
             C.c_float(float(shrink)), C.c_float(float(tversky_alpha)), C.c_float(float(tversky_beta)), K,
             self.block_cols, _ptr(self.w_idx), _ptr(self.w_val), _ptr(self.w_cnt), _ptr(self.t_indptr),
             _ptr(self.t_cols), _ptr(self.t_vals), _ptr(ws), int(nbytes.value), _stream())
        torch.cuda.current_stream().synchronize()      # the inputs and the workspace die with this frame

    def score(self, users, out=None):
        """S [B, I] float32 on the device: S[b] = sum over user b's train items j of r_uj W[j, :]"""
        dev = self.w_val.device
        if not isinstance(users, torch.Tensor):
            users = torch.from_numpy(np.ascontiguousarray(users, dtype=np.int32))
        users = users.to(dev, torch.int32).contiguous()
        B = int(users.numel())
        S = out if out is not None else torch.empty((B, self.n_items), dtype=torch.float32, device=dev)
        call("nrhip_itemknn_score", _ptr(users), B, _ptr(self.indptr), _ptr(self.indices), _ptr(self.ratings),
             self.n_users, self.n_items, _ptr(self.t_indptr), _ptr(self.t_cols), _ptr(self.t_vals),
             _ptr(S, torch.float32), S.stride(0), _stream())
        return S

    def similarity(self):
        """W as a host scipy CSR (float32): W[j, i] = the similarity of column i's neighbour j, as W_sparse"""
        idx, val, cnt = self.w_idx.cpu().numpy(), self.w_val.cpu().numpy(), self.w_cnt.cpu().numpy()
        keep = np.arange(self.neighbor)[None, :] < cnt[:, None]
        cols = np.broadcast_to(np.arange(self.n_items)[:, None], idx.shape)[keep]
        return sp.csr_matrix((val[keep], (idx[keep], cols)), shape=(self.n_items, self.n_items), dtype=np.float32)

    def scoring_csr(self):
        """W by rows, as the scoring kernel reads it: the transpose of the per-column lists, built on the device
        (host scipy CSR: row j = the columns whose list holds j, ascending)"""
        indptr = self.t_indptr.cpu().numpy()
        n = int(indptr[-1])
        return sp.csr_matrix((self.t_vals[:n].cpu().numpy(), self.t_cols[:n].cpu().numpy(), indptr),
                             shape=(self.n_items, self.n_items))
