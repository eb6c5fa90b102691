"""CDAE on the HIP engine: the batch loops of CDAE.py:108-140, the graph of CDAE.py:62-98 with one
`sess.run(self.train_opt)` per step, and predict() (csrc/cdae.hip).

A batch is a list of users.  Per user the device draws |R_u| num_neg items outside the train row R_u and keeps each
once; the decoder sees R_u (label 1) and those negatives (label 0), the encoder pools `en_embeddings` over the corrupted
union of both and adds the user's row and the offset.  Nothing of a batch returns to the host: its buffers are sized
from the bound |R_u| (1 + num_neg) per user, which the CSR gives.

Optimiser forms, as the TensorFlow stand-in's trace records them (tests/golden/make_golden_cdae.py): `user_embeddings`,
`de_embeddings` and `item_bias` are read through embedding_lookup / gather only and get the sparse application;
`en_embeddings`, read by sparse_tensor_dense_matmul as well, and `en_offset` get ApplyAdam.  Both forms move every row
and decay its moments every step; they differ in rounding only (neurec_amd/row_learner.py).
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import torch

from . import engine as E
from ._lib import CdaeBatchArgs, CdaeStepArgs, call
from .engine import _ptr, _stream
from .row_learner import RowLearner, addr, f32

MAX_D = 128                   # NRHIP_CDAE_MAX_D
MAX_BATCH = 1024              # NRHIP_CDAE_MAX_BATCH
SEGMENT_DRAWS = 16384         # NRHIP_CDAE_SEGMENT_DRAWS: a slot with more draws sends the batch through the one big sort
ACTS = {"identity": 0, "sigmoid": 1}
LOSSES = {"sigmoid_cross_entropy": 0, "square": 1}        # NR_POINT_CROSS_ENTROPY (summed here), NR_POINT_SQUARE
TABLES = ("user_embeddings", "en_embeddings", "en_offset", "de_embeddings", "de_bias")
_ROWS = ("user_embeddings", "de_embeddings", "de_bias")      # the sparse application
_DENSE = ("en_embeddings", "en_offset")                      # the dense one
_SHORT = {"user_embeddings": "user", "en_embeddings": "en", "en_offset": "offset", "de_embeddings": "de",
          "de_bias": "bias"}
_GOLDEN = 0x9e3779b97f4a7c15
_MASK64 = (1 << 64) - 1


def check_config(hidden_act, loss_func, num_neg, hidden_dim):
    """(activation code, loss code); the reference's two ValueErrors (CDAE.py:41, :94) and this engine's refusals"""
    if hidden_act not in ACTS:
        raise ValueError(f"hidden activate function {hidden_act} is invalid.")
    if loss_func not in LOSSES:
        raise ValueError("%s is an invalid loss function." % loss_func)
    if int(num_neg) < 1:
        raise ValueError("CDAE: num_neg=%d is not supported: with no negatives the decoder sees label 1 alone and the "
                         "input row is the train row; use num_neg >= 1" % int(num_neg))
    if int(hidden_dim) < 1 or int(hidden_dim) > MAX_D:
        raise NotImplementedError("CDAE: hidden_dim=%d is not supported (1 to %d)" % (int(hidden_dim), MAX_D))
    return ACTS[hidden_act], LOSSES[loss_func]


def _host_ids(x):
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32)


class CDAEBatch:
    """One batch on the device: users [B]; entry_ptr int64 [B + 1]; per decoder entry items, labels, slot and in_pos (the
    index of the entry's item in in_items); in_items, the input list.  The arrays hold `cap` entries, of which
    entry_ptr[B] are in use.  negatives(s) / host(): copies for tests and tools."""

    def __init__(self, h_users, users, entry_ptr, items, labels, slot, in_items, in_pos, cap, h_deg):
        self.h_users, self.users, self.entry_ptr, self.cap, self.h_deg = h_users, users, entry_ptr, int(cap), h_deg
        self.items, self.labels, self.slot, self.in_items, self.in_pos = items, labels, slot, in_items, in_pos
        self.B = len(h_users)

    def host(self):
        ptr = self.entry_ptr.cpu().numpy()
        n = int(ptr[-1])
        out = {"entry_ptr": ptr}
        for k in ("items", "labels", "slot", "in_items", "in_pos"):
            out[k] = getattr(self, k)[:n].cpu().numpy()
        return out

    def negatives(self):
        """per slot, the sorted de-duplicated negatives (host copies)"""
        h = self.host()
        return [h["items"][h["entry_ptr"][s] + self.h_deg[s]:h["entry_ptr"][s + 1]] for s in range(self.B)]


class CDAEEngine:
    """The five variables, their optimiser state and gradient buffers in HBM, and the train CSR.

    `step(users, loss_out, keep=None)`: build the batch of `users` (host ids), one gradient call, the applications.
    `score(users)` -> [B, I] on the device, corrupted like the reference's predict() unless keep_prob=1.0."""

    def __init__(self, tables, train, lr, reg, dropout, num_neg, max_batch, hidden_act="sigmoid",
                 loss_func="sigmoid_cross_entropy", learner="adam", seed=2018, momentum=0.9):
        T = {k: f32(tables[k]) for k in TABLES}
        if T["user_embeddings"].dim() != 2 or T["en_embeddings"].dim() != 2:
            raise ValueError("user_embeddings must be [num_users, hidden_dim], en_embeddings [num_items, hidden_dim]")
        (U, d), I = T["user_embeddings"].shape, T["en_embeddings"].shape[0]
        self.act, self.loss_kind = check_config(hidden_act, loss_func, num_neg, d)
        if tuple(T["en_embeddings"].shape) != (I, d) or tuple(T["de_embeddings"].shape) != (I, d) or \
                tuple(T["en_offset"].shape) != (d,) or tuple(T["de_bias"].shape) != (I,):
            raise ValueError("en_embeddings / de_embeddings must be [num_items, hidden_dim], en_offset [hidden_dim], "
                             "de_bias [num_items]")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError("CDAE: dropout=%r outside [0, 1)" % (dropout,))
        if int(max_batch) > MAX_BATCH:
            raise NotImplementedError("CDAE: batch_size=%d is not supported (up to %d users)" % (max_batch, MAX_BATCH))
        M = sp.csr_matrix(train)
        if M.shape != (U, I):
            raise ValueError("train matrix is %r, the tables say %r" % (M.shape, (U, I)))
        M.sum_duplicates()
        M.sort_indices()
        dev = E.require_gpu()
        self.hidden_act, self.loss_func, self.learner = hidden_act, loss_func, str(learner).lower()
        self.n_users, self.n_items, self.d = U, I, d
        self.csr = E.DeviceCSR.from_scipy(M)
        self.h_indptr = np.asarray(M.indptr, dtype=np.int64)
        self.h_indices = np.asarray(M.indices, dtype=np.int32)
        self.h_deg = np.diff(self.h_indptr)
        self.T = {k: t.contiguous().to(dev) for k, t in T.items()}
        self.G = {k: torch.zeros_like(t) for k, t in self.T.items()}
        self.lr, self.reg, self.keep_prob = float(lr), float(reg), float(np.float32(1.0) - np.float32(dropout))
        self.num_neg, self.max_batch, self.seed = int(num_neg), int(max_batch), int(seed)
        self.adam = E.AdamState(lr)
        self.opt = RowLearner(self.learner, lr, momentum, self.adam)
        slots = {k: self.opt.slots(t) for k, t in self.T.items()}
        self.s0, self.s1 = ({k: s[i] for k, s in slots.items()} for i in (0, 1))
        self.flag = {k: self.opt.flag(self.T[k].shape[0], dev) for k in _ROWS}
        B = max(self.max_batch, 1)
        self._hidden = torch.empty((B, d), dtype=torch.float32, device=dev)
        self._dz = torch.empty((B, d), dtype=torch.float32, device=dev)
        self._scal = torch.empty(4 * B, dtype=torch.float32, device=dev)
        self._cap = 0
        self._keys = self._g = self._l2 = None
        self.t = 0                                             # steps applied
        self._score_calls = 0
        self.last_keep = None                                  # the mask of the last gradients() / hidden() call
        self._items = None                                     # (step, [de_embeddings | de_bias])
        self._gemm = None                                      # [the scoring GEMM, the step its items were prepared at]

    # ------------------------------------------------------------------ batches
    def _users(self, users):
        h = _host_ids(users)
        if len(h) > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if len(h) and (h.min() < 0 or h.max() >= self.n_users):
            raise ValueError("CDAE: user ids must lie in [0, %d)" % self.n_users)
        return h

    def batch(self, users, seed):
        """the batch of `users` (host ids, repeats allowed) with the negatives of `seed`, built on the device"""
        h = self._users(users)
        B, dev = len(h), self.T["en_offset"].device
        deg = self.h_deg[h].astype(np.int64)
        pos_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        P, nn = int(pos_ptr[-1]), self.num_neg
        cap = P * (1 + nn)
        if cap + B > 1 << 30:                                  # the step sorts cap + B keys (nrhip_sort_u64's limit)
            raise NotImplementedError("CDAE: a batch of %d entries is not supported" % cap)
        meta64 = torch.from_numpy(np.concatenate([pos_ptr, pos_ptr * nn])).to(dev)
        meta32 = torch.from_numpy(np.concatenate([h, (deg * nn).astype(np.int32)]).astype(np.int32)).to(dev)
        users_d = meta32[:B]
        entry_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        n = max(cap, 1)
        items, slot, in_items, in_pos = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
        labels = torch.empty(n, dtype=torch.float32, device=dev)
        out = CDAEBatch(h, users_d, entry_ptr, items, labels, slot, in_items, in_pos, cap, deg)
        if B == 0:
            return out
        keys = torch.empty(max(P * nn, 1), dtype=torch.int64, device=dev)
        a = CdaeBatchArgs()
        a.indptr, a.indices = _ptr(self.csr.indptr, torch.int64), _ptr(self.csr.indices, torch.int32)
        a.users, a.pos_ptr, a.seg_off = _ptr(users_d), C.c_void_p(meta64.data_ptr()), \
            C.c_void_p(meta64.data_ptr() + 8 * (B + 1))
        a.seg_len = C.c_void_p(meta32.data_ptr() + 4 * B)
        a.keys, a.entry_ptr = _ptr(keys), _ptr(entry_ptr)
        a.items, a.labels, a.slot, a.in_items, a.in_pos = (_ptr(t) for t in (items, labels, slot, in_items, in_pos))
        a.n_draws, a.seed = P * nn, int(seed) & _MASK64
        a.n_users, a.n_items, a.batch, a.num_neg = self.n_users, self.n_items, B, nn
        a.max_draws = int(deg.max()) * nn if B else 0
        call("nrhip_cdae_batch", C.byref(a), _stream())
        out._keep_alive = (meta64, meta32, keys)
        return out

    def batch_given(self, users, negatives):
        """the batch of `users` with these negatives per slot (ascending, distinct, outside the train row), laid out on
        the host: for traces that record the reference's own draws"""
        h = self._users(users)
        B, dev = len(h), self.T["en_offset"].device
        if len(negatives) != B:
            raise ValueError("one list of negatives per user")
        ptr, items, labels, slot, in_items, in_pos = [0], [], [], [], [], []
        for s, u in enumerate(h):
            row = self.h_indices[self.h_indptr[u]:self.h_indptr[u + 1]]
            neg = np.asarray(negatives[s], dtype=np.int32).reshape(-1)
            if len(neg) and (np.any(np.diff(neg) <= 0) or neg[0] < 0 or neg[-1] >= self.n_items or
                             np.intersect1d(neg, row).size):
                raise ValueError("negatives of slot %d must ascend strictly inside [0, %d) and outside the train row"
                                 % (s, self.n_items))
            dec = np.concatenate([row, neg])
            order = np.argsort(dec, kind="stable")
            place = np.empty(len(dec), np.int64)
            place[order] = np.arange(len(dec))
            items.append(dec)
            labels.append(np.concatenate([np.ones(len(row), np.float32), np.zeros(len(neg), np.float32)]))
            slot.append(np.full(len(dec), s, np.int32))
            in_items.append(dec[order])
            in_pos.append(ptr[-1] + place)
            ptr.append(ptr[-1] + len(dec))

        def up(parts, dtype):
            flat = np.concatenate(parts).astype(dtype) if parts and ptr[-1] else np.zeros(1, dtype)
            return torch.from_numpy(flat).to(dev)
        return CDAEBatch(h, torch.from_numpy(h if B else np.zeros(1, np.int32)).to(dev)[:B],
                         torch.from_numpy(np.asarray(ptr, np.int64)).to(dev), up(items, np.int32),
                         up(labels, np.float32), up(slot, np.int32), up(in_items, np.int32), up(in_pos, np.int32),
                         ptr[-1], self.h_deg[h].astype(np.int64))

    def _keep(self, keep, n, dev):
        """(uint8 device tensor of n entries at least, given flag)"""
        if keep is None:
            return torch.empty(max(n, 1), dtype=torch.uint8, device=dev), 0
        if not isinstance(keep, torch.Tensor):
            keep = torch.from_numpy(np.ascontiguousarray(np.asarray(keep).reshape(-1), dtype=np.uint8))
        keep = keep.to(dev, torch.uint8).contiguous()
        if keep.numel() < n:
            keep = torch.cat([keep, torch.zeros(n - keep.numel(), dtype=torch.uint8, device=dev)])
        return keep, 1

    # ------------------------------------------------------------------ the step
    def gradients(self, batch, loss_out, keep=None):
        """the C call alone: loss_out and the batch's rows of self.G (and the row flags); no table moves.  keep: uint8
        per input entry of the batch (None: drawn from (seed, step) and left in self.last_keep)"""
        B, cap, dev = batch.B, batch.cap, self.T["en_offset"].device
        if B == 0:
            return
        if self._keys is None or self._cap < cap:
            self._cap = cap
            self._keys = torch.empty(cap + max(self.max_batch, 1), dtype=torch.int64, device=dev)
            self._l2 = torch.empty(cap + max(self.max_batch, 1), dtype=torch.float32, device=dev)
            self._g = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
        keep, given = self._keep(keep, cap, dev)
        a = CdaeStepArgs()
        for k in TABLES:
            setattr(a, _SHORT[k], _ptr(self.T[k]))
            setattr(a, "G_" + _SHORT[k], _ptr(self.G[k]))
        for k in _ROWS:
            setattr(a, "flag_" + _SHORT[k], addr(self.flag[k]))
        a.users, a.entry_ptr = _ptr(batch.users, torch.int32), _ptr(batch.entry_ptr, torch.int64)
        a.items, a.labels, a.slot = _ptr(batch.items), _ptr(batch.labels), _ptr(batch.slot)
        a.in_items, a.in_pos, a.keep = _ptr(batch.in_items), _ptr(batch.in_pos), _ptr(keep)
        a.keys, a.g, a.hidden, a.dz = _ptr(self._keys), _ptr(self._g), _ptr(self._hidden), _ptr(self._dz)
        a.scal, a.l2, a.loss2 = _ptr(self._scal), _ptr(self._l2), _ptr(loss_out, torch.float32)
        a.seed, a.step = self.seed & _MASK64, self.t
        a.n_users, a.n_items, a.d, a.batch, a.entry_cap = self.n_users, self.n_items, self.d, B, cap
        a.act, a.loss_kind, a.keep_given = self.act, self.loss_kind, given
        a.keep_prob, a.reg = self.keep_prob, self.reg
        call("nrhip_cdae_step", C.byref(a), _stream())
        self.last_keep = keep

    def apply(self):
        """the five applications of self.G; the gradients (and flags) are zero again afterwards"""
        for k in _ROWS:
            self.opt.apply(self.T[k], self.s0[k], self.s1[k], self.G[k], self.flag[k])
        self.opt.apply_dense([(self.T[k], self.s0[k], self.s1[k], self.G[k]) for k in _DENSE], clear_grad=True)
        self.adam.advance()
        self.t += 1

    def step_seed(self):
        """the seed of the next step's draws"""
        return (self.seed + _GOLDEN * (self.t + 1)) & _MASK64

    def step(self, users, loss_out, keep=None, negatives=None):
        """one batch of users (host ids).  loss_out: 2 floats on the device, (loss term, regulariser term) before the
        update.  negatives: per-slot lists instead of the device's draws.  An empty batch is a no-op."""
        if len(users) == 0:
            return
        batch = self.batch(users, self.step_seed()) if negatives is None else self.batch_given(users, negatives)
        self.gradients(batch, loss_out, keep)
        self.apply()

    # ------------------------------------------------------------------ scoring
    def factors(self, users, keep=None, keep_prob=None):
        """[B, d + 1] rows [hidden | 1] of `users` (host ids) from their train rows; keep: uint8 per train entry of the
        users in order (None: drawn, left in self.last_keep); keep_prob: None = 1 - dropout"""
        h = _host_ids(users)
        B, dev = len(h), self.T["en_offset"].device
        if B and (h.min() < 0 or h.max() >= self.n_users):
            raise ValueError("CDAE: user ids must lie in [0, %d)" % self.n_users)
        kp = self.keep_prob if keep_prob is None else float(keep_prob)
        if not 0.0 < kp <= 1.0:
            raise ValueError("CDAE: keep_prob=%r outside (0, 1]" % (keep_prob,))
        out = torch.empty((B, self.d + 1), dtype=torch.float32, device=dev)
        mask_ptr = np.concatenate([[0], np.cumsum(self.h_deg[h])]).astype(np.int64)
        if kp >= 1.0:
            keep_t, given, ptr_d = None, 0, None
        else:
            keep_t, given = self._keep(keep, int(mask_ptr[-1]), dev)
            ptr_d = torch.from_numpy(mask_ptr).to(dev)
        self._score_calls += 1
        call("nrhip_cdae_user_factors", _ptr(self.csr.indptr), _ptr(self.csr.indices), self.n_users, self.n_items,
             _ptr(self.T["user_embeddings"]), _ptr(self.T["en_embeddings"]), _ptr(self.T["en_offset"]), self.d,
             self.act, _ptr(torch.from_numpy(h).to(dev) if B else None, allow_none=True),
             _ptr(ptr_d, allow_none=True), B, _ptr(keep_t, allow_none=True), given, C.c_float(kp),
             (self.seed + 1) & _MASK64, self._score_calls, _ptr(out), out.stride(0), _stream())
        self.last_keep = keep_t
        return out

    def hidden(self, users, keep=None, keep_prob=None):
        """[B, d]: the encoder's output for `users` on their train rows"""
        return self.factors(users, keep, keep_prob)[:, :self.d]

    def item_factors(self):
        """[I, d + 1] rows [de_embeddings[i] | de_bias[i]]"""
        if self._items is None or self._items[0] != self.t:
            self._items = (self.t, torch.cat([self.T["de_embeddings"], self.T["de_bias"].reshape(-1, 1)],
                                             dim=1).contiguous())
        return self._items[1]

    def score(self, users, keep=None, keep_prob=None):
        """S [B, I] float32 on the device: CDAE.py:148-160 for `users`, every item"""
        F = self.factors(users, keep, keep_prob)
        items, B = self.item_factors(), int(F.shape[0])
        if B == 0:
            return torch.empty((0, self.n_items), dtype=torch.float32, device=F.device)
        if self._gemm is None or self._gemm[0].max_rows < B:
            self._gemm = [E.score_gemm_for(items, max(B, 1)), self.t]
        elif self._gemm[1] != self.t:                          # the item side is prepared once per table state
            self._gemm[0].prepare(items)
            self._gemm[1] = self.t
        return self._gemm[0](F, None)[:, :self.n_items]

    def forward(self, users, items, sizes=None, keep=None, keep_prob=None):
        """candidate mode: the scores of the flat `items`, sizes[b] of them for users[b] (None: one each), on the
        device; every user is encoded once"""
        F = self.factors(users, keep, keep_prob)
        it = _host_ids(items)
        sizes = np.ones(F.shape[0], np.int64) if sizes is None else np.asarray(sizes, dtype=np.int64)
        if int(sizes.sum()) != len(it) or len(sizes) != F.shape[0]:
            raise ValueError("sizes must hold one count per user and sum to the number of items")
        dev = F.device
        out = torch.empty(len(it), dtype=torch.float32, device=dev)
        if len(it) == 0:
            return out
        rows = torch.from_numpy(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)).to(dev)
        call("nrhip_cdae_pairs", _ptr(F), F.stride(0), _ptr(self.T["de_embeddings"]), _ptr(self.T["de_bias"]),
             self.n_items, self.d, _ptr(rows), _ptr(torch.from_numpy(it).to(dev)), len(it), _ptr(out), _stream())
        return out

    def tables(self):
        """{name: numpy copy} of the five variables"""
        return {k: t.cpu().numpy() for k, t in self.T.items()}
