"""JCA on the HIP engine: the pairs of one block of the rating matrix (JCA.py:179-200), one `sess.run([optimizer,
cost])` per block (JCA.py:80-116, 150-159) and the ratings of `evaluate()` (JCA.py:167-176) — csrc/jca.hip.

Rows r are the batch users (Bu), columns c the batch items (Bi), H = hidden_neuron:
    hu[a]  = g(sum over i in R[r_a,:] of UV[i,:] + Ub1)
    hi[b]  = g((sum over u in R[:,c_b] of IV[u,:] + Ib1) * I_factor_vector[c_b])
    D[a,b] = (f(hu[a] . UW[:,c_b] + Ub2[c_b]) + f(hi[b] . IW[:,r_a] + Ib2[r_a])) / 2
    cost   = sum over pairs (a, bp, bn) of max(0, D[a,bn] - D[a,bp] + margin)
             + reg * 0.5 * sum over {UW, UV, IW, IV, Ib1, Ib2, Ub1, Ub2} of sum(w^2) / 2
The encoders pool table rows over the CSR row and the CSC column: no [B, I] or [U, B] slab is formed.  A pair is active
when its hinge argument is > 0.

Layout.  All nine variables, their Adam slots and their gradients lie at the same offsets of four flat device arrays in
the order UV [I, H], UW transposed [I, H], IV [U, H], IW transposed [U, H], Ub2 [I], I_factor_vector [I], Ib2 [U],
Ub1 [H], Ib1 [H]; `tables()` gives the reference's names and shapes.

Optimiser forms, as TF-1.12 picks them: every variable is consumed by matmul, so the dense application moves all of
every variable at each step; under Adam a row without a gradient still moves.  The regulariser's gradient 0.5 reg w
rides on the sweep.  I_factor_vector is trained and not regularised.
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from ._lib import JcaArgs, call
from .engine import _ptr, _stream

MAX_H = 128                   # NRHIP_JCA_MAX_H
MAX_BATCH = 512               # NRHIP_JCA_MAX_BATCH
MAX_NEG = 8                   # NRHIP_JCA_MAX_NEG
ACTIVATIONS = ("sigmoid", "tanh", "relu", "elu", "identity")      # NRHIP_JCA_ACT_*: the position is the code
LEARNERS = ("adam", "gd")
NAMES = ("UV", "UW", "Ub1", "Ub2", "IV", "IW", "Ib1", "Ib2", "I_factor_vector")      # the reference's creation order


def check_config(hidden_neuron, batch_size, num_neg, f_act, g_act, learner, margin, reg, learning_rate):
    """the refusals, each with its key and the supported range"""
    def rng(key, val, lo, hi):
        if int(val) != val or val < lo or val > hi:
            raise NotImplementedError("JCA: %s=%r is not supported (%d to %d)" % (key, val, lo, hi))
    rng("hidden_neuron", hidden_neuron, 1, MAX_H)
    rng("batch_size", batch_size, 1, MAX_BATCH)
    rng("num_neg", num_neg, 1, MAX_NEG)
    for key, val in (("f_act", f_act), ("g_act", g_act)):
        if val not in ACTIVATIONS:
            raise NotImplementedError("JCA: %s=%r is not supported (one of %s; softmax needs the whole row and selu is "
                                      "left out)" % (key, val, ", ".join(ACTIVATIONS)))
    if str(learner).lower() not in LEARNERS:
        raise NotImplementedError("JCA: learner=%r is not supported (one of %s)" % (learner, ", ".join(LEARNERS)))
    if not margin >= 0:
        raise ValueError("JCA: margin=%r is not supported (margin >= 0)" % (margin,))
    if not reg >= 0:
        raise ValueError("JCA: reg=%r is not supported (reg >= 0)" % (reg,))
    if not learning_rate > 0:
        raise ValueError("JCA: learning_rate=%r is not supported (learning_rate > 0)" % (learning_rate,))


def check_train_values(train_csr):
    """the refusal of a train matrix with a stored value other than 1"""
    data = np.asarray(train_csr.data)
    bad = np.flatnonzero(data != 1)
    if bad.size:
        raise ValueError("JCA: the train matrix holds the value %r; only stored values of 1 are supported (the "
                         "reference would take the entries equal to 1 as positives and feed the ratings as input)"
                         % (data[bad[0]].item(),))


def pack_pairs(p, n):
    """[n, 2] (block row, block column) of the positives and of the negatives -> the device's pair words"""
    p, n = np.asarray(p, dtype=np.int64).reshape(-1, 2), np.asarray(n, dtype=np.int64).reshape(-1, 2)
    if p.shape != n.shape or np.any(p[:, 0] != n[:, 0]):
        raise ValueError("pairs_given: positives and negatives must pair up row by row")
    return ((p[:, 0] << 18) | (p[:, 1] << 9) | n[:, 1]).astype(np.uint32)


def unpack_pairs(words):
    """pair words -> (block row, positive column, negative column) int64 arrays"""
    w = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    return w >> 18, (w >> 9) & 511, w & 511


class JCAPairs:
    """the pair list of one block on the device: `words` uint32 (as int32 storage) [n]"""

    def __init__(self, words, n, rows=None, cols=None):
        self.words, self.n = words, int(n)
        self.rows, self.cols = rows, cols                   # the block's checked ids on the device

    def numpy(self):
        return unpack_pairs(self.words[:self.n].cpu().numpy().view(np.uint32))


class JCAEngine:
    """The nine variables, their optimiser slots and gradient buffers, the train CSR and CSC in HBM.

    `pairs(rows, cols, epoch, i, j)` / `pairs_given(rows, cols, p, n)` -> JCAPairs; `step(rows, cols, pairs, loss)` one
    block step (loss: 2 floats on the device, the hinge term and the regulariser term before the update; a block
    without pairs moves nothing, the Adam step count included); `encode_items()` then `score(users)` -> [n, I] and
    `score_pairs(users, items)` -> [n]; `tables()` the variables under the reference's names and shapes."""

    def __init__(self, variables, train_csr, hidden_neuron, batch_size, num_neg=1, f_act="tanh", g_act="tanh",
                 learner="adam", learning_rate=0.001, reg=0.0, margin=0.15, seed=2019):
        check_config(hidden_neuron, batch_size, num_neg, f_act, g_act, learner, margin, reg, learning_rate)
        csr = train_csr.tocsr().copy()
        csr.sum_duplicates()
        csr.sort_indices()
        check_train_values(csr)
        U, I = csr.shape
        H = int(hidden_neuron)
        shapes = {"UV": (I, H), "UW": (H, I), "Ub1": (1, H), "Ub2": (1, I), "IV": (U, H), "IW": (H, U), "Ib1": (1, H),
                  "Ib2": (1, U), "I_factor_vector": (1, I)}
        for k in NAMES:
            if tuple(np.shape(variables[k])) != shapes[k]:
                raise ValueError("JCA: %s must be %r, got %r" % (k, shapes[k], tuple(np.shape(variables[k]))))
        self.dev = dev = E.require_gpu()
        self.n_users, self.n_items, self.H = U, I, H
        self.batch_size, self.num_neg = int(batch_size), int(num_neg)
        self.f_act, self.g_act = ACTIVATIONS.index(f_act), ACTIVATIONS.index(g_act)
        self.learner = str(learner).lower()
        self.lr, self.reg, self.margin = float(learning_rate), float(reg), float(margin)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.adam = E.AdamState(learning_rate)
        self.t = 0
        # the flat layout of include/neurec_hip.h
        self._off, o = {}, 0
        for k, n in (("UV", I * H), ("UW", I * H), ("IV", U * H), ("IW", U * H), ("Ub2", I), ("I_factor_vector", I),
                     ("Ib2", U), ("Ub1", H), ("Ib1", H)):
            self._off[k] = (o, n)
            o += n
        host = np.empty(o, dtype=np.float32)
        for k in NAMES:
            v = np.asarray(variables[k], dtype=np.float32)
            b, n = self._off[k]
            host[b:b + n] = (v.T if k in ("UW", "IW") else v).reshape(-1)
        self.W = torch.from_numpy(host).to(dev)
        self.M, self.V, self.G = (torch.zeros_like(self.W) for _ in range(3))
        self.flag = torch.zeros(4 * I + 3 * U, dtype=torch.uint8, device=dev)
        csc = csr.tocsc()
        csc.sort_indices()
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        self.indptr, self.indices = to(csr.indptr, np.int64), to(csr.indices, np.int32)
        self.t_indptr, self.t_users = to(csc.indptr, np.int64), to(csc.indices, np.int32)
        self.rowslot = torch.zeros(U, dtype=torch.int64, device=dev)
        self.colslot = torch.zeros(I, dtype=torch.int64, device=dev)
        sizes = (C.c_int64 * 4)()
        call("nrhip_jca_workspace", U, I, H, self.batch_size, self.num_neg, C.cast(sizes, C.c_void_p))
        self._wsf = torch.empty(sizes[0], dtype=torch.float32, device=dev)
        self._wsi = torch.empty(sizes[1], dtype=torch.int32, device=dev)
        self._wsd = torch.empty(sizes[2], dtype=torch.float64, device=dev)
        self.max_pairs = int(sizes[3])
        self._total = torch.zeros(1, dtype=torch.int32, device=dev)
        self._loss_scratch = torch.zeros(2, dtype=torch.float32, device=dev)
        self._stamp = 0
        self.hi = None                                      # [I, H] of encode_items(); None: stale

    # ------------------------------------------------------------------ helpers
    def _ids(self, x, high, what, distinct=True, limit=None):
        """host ids checked against [0, high) (and for repeats) -> int32 on the device; they index tables"""
        if isinstance(x, torch.Tensor):
            x = x.cpu().numpy()
        x = np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int64)
        if x.size and (x.min() < 0 or x.max() >= high):
            raise ValueError("JCA: %s outside [0, %d)" % (what, high))
        if limit is not None and x.size > limit:
            raise ValueError("JCA: %d %s, at most batch_size=%d" % (x.size, what, limit))
        if distinct and np.unique(x).size != x.size:
            raise ValueError("JCA: %s must be distinct" % what)
        return torch.from_numpy(x.astype(np.int32)).to(self.dev)

    def _args(self, rows=None, cols=None):
        a = JcaArgs()
        a.W, a.M, a.V, a.G, a.flag = (_ptr(t) for t in (self.W, self.M, self.V, self.G, self.flag))
        a.indptr, a.indices, a.t_indptr, a.t_users = (_ptr(t) for t in (self.indptr, self.indices, self.t_indptr,
                                                                        self.t_users))
        a.rowslot, a.colslot = _ptr(self.rowslot), _ptr(self.colslot)
        a.wsf, a.wsi, a.wsd = _ptr(self._wsf), _ptr(self._wsi), _ptr(self._wsd)
        a.total, a.loss2 = _ptr(self._total), _ptr(self._loss_scratch)
        a.seed = self.seed
        a.n_users, a.n_items, a.H = self.n_users, self.n_items, self.H
        a.batch_size, a.num_neg, a.f_act, a.g_act = self.batch_size, self.num_neg, self.f_act, self.g_act
        a.margin, a.reg = self.margin, self.reg
        if rows is not None:
            self._stamp += 1
            if self._stamp >= 2 ** 31 - 1:                  # the slot maps hold the stamp in 31 bits: start over
                self.rowslot.zero_()
                self.colslot.zero_()
                self._stamp = 1
            a.stamp = self._stamp
            a.rows, a.cols, a.n_rows, a.n_cols = _ptr(rows), _ptr(cols), int(rows.numel()), int(cols.numel())
        return a

    def block(self, rows, cols):
        """(rows, cols) of a block, checked, as int32 device tensors"""
        return (self._ids(rows, self.n_users, "block rows", limit=self.batch_size),
                self._ids(cols, self.n_items, "block columns", limit=self.batch_size))

    # ------------------------------------------------------------------ pairs
    def pairs(self, rows, cols, epoch, i, j):
        """the block's pairs: a pure function of (seed, epoch, i, j) and the block.  One copy of 4 bytes to the host."""
        rows, cols = self.block(rows, cols)
        words = torch.empty(self.max_pairs, dtype=torch.int32, device=self.dev)
        if rows.numel() == 0 or cols.numel() == 0:
            return JCAPairs(words, 0, rows, cols)
        a = self._args(rows, cols)
        a.pairs = _ptr(words)
        a.epoch, a.block_i, a.block_j = int(epoch) & 0xFFFFFFFFFFFFFFFF, int(i), int(j)
        call("nrhip_jca_pairs", C.byref(a), _stream())
        return JCAPairs(words, int(self._total.item()), rows, cols)

    def pairs_given(self, rows, cols, p, n):
        """recorded pairs: p and n [n_pairs, 2] of (block row, block column), as the reference's p_input / n_input"""
        rows, cols = self.block(rows, cols)
        words = pack_pairs(p, n)
        ar, bp, bn = unpack_pairs(words)
        if words.size and (ar.max() >= rows.numel() or max(bp.max(), bn.max()) >= cols.numel() or
                           min(np.min(p), np.min(n)) < 0):
            raise ValueError("pairs_given: a pair lies outside the block")
        if words.size > self.max_pairs:
            raise ValueError("pairs_given: %d pairs, at most %d" % (words.size, self.max_pairs))
        return JCAPairs(torch.from_numpy(words.view(np.int32)).to(self.dev), words.size, rows, cols)

    # ------------------------------------------------------------------ training
    def gradients(self, rows, cols, pairs, loss_out):
        """the gradient call alone: loss_out[0] and the touched rows of G with their flags; no variable moves.  The
        pairs carry their block's ids, checked when they were made; `rows` and `cols` must be that block."""
        if pairs.rows is None or len(rows) != pairs.rows.numel() or len(cols) != pairs.cols.numel():
            raise ValueError("JCA: the pairs were made for another block")
        rows, cols = pairs.rows, pairs.cols
        a = self._args(rows, cols)
        a.pairs, a.n_pairs, a.loss2 = _ptr(pairs.words), pairs.n, _ptr(loss_out, torch.float32)
        call("nrhip_jca_step", C.byref(a), _stream())

    def apply(self, loss_out):
        """the sweep over all nine variables; loss_out[1] = the regulariser term of the variables as they come in.  The
        gradient buffers and flags are zero again afterwards."""
        a = self._args()
        a.loss2 = _ptr(loss_out, torch.float32)
        adam = self.learner == "adam"
        step = float(self.adam.alpha()) if adam else self.lr
        call("nrhip_jca_apply", C.byref(a), int(adam), step, float(self.adam.beta1), float(self.adam.beta2),
             float(self.adam.eps), _stream())
        self.adam.advance()
        self.t += 1
        self.hi = None

    def step(self, rows, cols, pairs, loss_out):
        """one block step.  A block without pairs is skipped: no optimiser step, loss 0."""
        if pairs.n == 0:
            loss_out.zero_()
            return
        self.gradients(rows, cols, pairs, loss_out)
        self.apply(loss_out)

    # ------------------------------------------------------------------ scoring
    def encode(self, which, ids=None):
        """hu of the users `ids` (which = 0) or hi of the items (which = 1); ids None: all of them"""
        n_all = self.n_items if which else self.n_users
        ids = None if ids is None else self._ids(ids, n_all, "ids", distinct=False)
        n = n_all if ids is None else int(ids.numel())
        out = torch.empty((n, self.H), dtype=torch.float32, device=self.dev)
        a = self._args()
        call("nrhip_jca_encode", C.byref(a), int(which), _ptr(ids, allow_none=True), n, _ptr(out), _stream())
        return out

    def encode_items(self):
        """hi of every item, [I, H]: once per evaluate(); a step makes it stale"""
        self.hi = self.encode(1)
        return self.hi

    def score(self, users):
        """D [n, I] float32 on the device for `users` against every item"""
        if self.hi is None:
            self.encode_items()
        users = self._ids(users, self.n_users, "users", distinct=False)
        n = int(users.numel())
        out = torch.empty((n, self.n_items), dtype=torch.float32, device=self.dev)
        if n == 0:
            return out
        hu = torch.empty((n, self.H), dtype=torch.float32, device=self.dev)
        a = self._args()
        call("nrhip_jca_encode", C.byref(a), 0, _ptr(users), n, _ptr(hu), _stream())
        call("nrhip_jca_score", C.byref(a), _ptr(users), n, _ptr(hu), _ptr(self.hi), _ptr(out), self.n_items, _stream())
        return out

    def score_pairs(self, users, items):
        """D [n] float32 on the device of the (user, item) pairs"""
        if self.hi is None:
            self.encode_items()
        if isinstance(users, torch.Tensor):
            users = users.cpu().numpy()
        users = np.asarray(users).reshape(-1)
        uniq, inverse = np.unique(users, return_inverse=True)
        d_users = self._ids(users, self.n_users, "users", distinct=False)
        d_items = self._ids(items, self.n_items, "items", distinct=False)
        n = int(d_users.numel())
        if d_items.numel() != n:
            raise ValueError("score_pairs: users and items must have the same length")
        out = torch.empty(n, dtype=torch.float32, device=self.dev)
        if n == 0:
            return out
        hu = self.encode(0, uniq)
        slot = torch.from_numpy(inverse.astype(np.int32)).to(self.dev)
        a = self._args()
        call("nrhip_jca_score_pairs", C.byref(a), _ptr(d_users), _ptr(d_items), _ptr(slot), n, _ptr(hu), _ptr(self.hi),
             _ptr(out), _stream())
        return out

    # ------------------------------------------------------------------ views
    def _view(self, flat, k):
        b, n = self._off[k]
        v = flat[b:b + n]
        if k in ("UV", "IV"):
            return v.view(-1, self.H)
        if k in ("UW", "IW"):
            return v.view(-1, self.H).t()
        return v.view(1, -1)

    def tables(self):
        """{name: float32 array} under the reference's names and shapes"""
        return {k: self._view(self.W, k).contiguous().cpu().numpy() for k in NAMES}

    def gradient_tables(self):
        """the gradient buffers in the same form (all zero between steps)"""
        return {k: self._view(self.G, k).contiguous().cpu().numpy() for k in NAMES}
