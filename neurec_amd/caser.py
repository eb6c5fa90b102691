"""Caser on the HIP engine: the graph of model/sequential_recommender/Caser.py:70-122, one `sess.run(self.train_opt)` per
step, and predict() (csrc/caser.hip).

Variables in creation order (the layers create theirs at their first call in build_graph): user_embeddings [U, d],
seq_item_embeddings [I, d] (read through a concat with a zero pad row I), item_embeddings [I, 2d], item_biases [I],
conv_v_kernel [L, nv] (the Conv2D kernel [L, 1, 1, nv]) and conv_v_bias [nv], for the heights i = 1..L conv_h<i>_kernel
[i, d, nh] (the kernel [i, d, 1, nh]) and conv_h<i>_bias [nh], fc1_kernel [F, d] and fc1_bias [d]; F = nv d + nh L.

Optimiser forms, as TF-1.12 picks them (Adam 0.9 / 0.999 / 1e-8).  With l2_reg != 0 the regulariser's dense gradient
joins each gather's and all four tables take ApplyAdam over every row.  With l2_reg == 0 user_embeddings,
item_embeddings and item_biases are gathered from the variable — Adam's sparse form, which sweeps every row (the note in
neurec_amd/gru4rec.py) — and seq_item_embeddings, read through the concat, has a dense gradient: ApplyAdam.  The conv and
dense variables are dense in both cases and have no regulariser.

Dropout over the F features: `mask` given as a uint8 [B, F] device tensor, or a counter-based device generator keyed by
(seed, step, element).

The pad row I of the sequence table is zero and takes no gradient.  A pad id among the positives (a user with fewer than
seq_T train items) has logit 0 and no gradient and stays in the mean's denominator: TF on a GPU reads zeros there.
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from ._lib import CaserStepArgs, CaserWeights, call
from .engine import _ptr, _stream
from .row_learner import as_ids, f32

MAX_WIDTH = 128               # NRHIP_CASER_MAX_WIDTH
MAX_LEN = 10                  # NRHIP_CASER_MAX_LEN
MAX_NV = 16                   # NRHIP_CASER_MAX_NV
MAX_NH = 64                   # NRHIP_CASER_MAX_NH
MAX_TARGETS = 16              # NRHIP_CASER_MAX_TARGETS
MAX_BATCH = 4096              # NRHIP_CASER_MAX_BATCH
SCORES_MAX_WIDTH = 128        # NRHIP_GRU4REC_MAX_WIDTH: nrhip_gru4rec_scores' widest row; beyond it nrhip_caser_scores
TABLES = ("user_embeddings", "seq_item_embeddings", "item_embeddings", "item_biases")
SPARSE_FORM = ("user_embeddings", "item_embeddings", "item_biases")       # at l2_reg == 0
# variable -> its field in nrhip_caser_weights (the gradient's in nrhip_caser_step_args: G_ in front)
FIELDS = {"user_embeddings": "user", "seq_item_embeddings": "seq_item", "item_embeddings": "item",
          "item_biases": "item_bias", "conv_v_kernel": "conv_v", "conv_v_bias": "conv_v_bias", "fc1_kernel": "fc",
          "fc1_bias": "fc_bias"}


def table_names(seq_L):
    out = list(TABLES) + ["conv_v_kernel", "conv_v_bias"]
    for i in range(1, seq_L + 1):
        out += ["conv_h%d_kernel" % i, "conv_h%d_bias" % i]
    return out + ["fc1_kernel", "fc1_bias"]


def _limit(name, value, hi):
    if not 1 <= value <= hi:
        raise NotImplementedError("Caser: %s=%d is not supported (1 to %d)" % (name, value, hi))


class CaserEngine:
    """Tables, optimiser slots and gradient buffers in HBM.

    `variables`: {name: array} of table_names(seq_L).  `step(users, seq, pos, neg, loss_out)`: one batch — users int32
    [B], seq [B, L], pos [B, T], neg [B, N], the pad item id I — gradients, then Adam.  `run_schedule` issues a whole
    epoch.  `forward_rows(users, seq)` -> concat(z, user row) with training off; `score(users)` -> [n, I] on the
    device."""

    def __init__(self, variables, lr, l2_reg, max_batch, seq_T, neg_samples, nv, nh, dropout_rate, seed=2017):
        user, seq_item = f32(variables["user_embeddings"]), f32(variables["seq_item_embeddings"])
        if user.dim() != 2 or seq_item.dim() != 2 or user.shape[1] != seq_item.shape[1]:
            raise ValueError("user_embeddings must be [users_num, factors_num], seq_item_embeddings [items_num, "
                             "factors_num]")
        U, I, d = int(user.shape[0]), int(seq_item.shape[0]), int(user.shape[1])
        L = (len(variables) - 8) // 2
        T, N, nv, nh, max_batch = int(seq_T), int(neg_samples), int(nv), int(nh), int(max_batch)
        _limit("factors_num", d, MAX_WIDTH)
        _limit("seq_L", L, MAX_LEN)
        _limit("nv", nv, MAX_NV)
        _limit("nh", nh, MAX_NH)
        _limit("seq_T", T, MAX_TARGETS)
        _limit("neg_samples", N, MAX_TARGETS)
        if max_batch < 1:
            raise ValueError("max_batch must be at least 1")
        if max_batch > MAX_BATCH:
            raise NotImplementedError("Caser: max_batch=%d is not supported (1 to %d)" % (max_batch, MAX_BATCH))
        if U + 2 * I >= 1 << 31:
            raise NotImplementedError("Caser: users_num + 2 items_num = %d is not supported (below 2^31)" % (U + 2 * I))
        if not 0.0 <= float(dropout_rate) < 1.0:
            raise ValueError("Caser: dropout=%r outside [0, 1)" % (dropout_rate,))
        F = nv * d + nh * L
        shapes = {"user_embeddings": (U, d), "seq_item_embeddings": (I, d), "item_embeddings": (I, 2 * d),
                  "item_biases": (I,), "conv_v_kernel": (L, nv), "conv_v_bias": (nv,), "fc1_kernel": (F, d),
                  "fc1_bias": (d,)}
        for i in range(1, L + 1):
            shapes["conv_h%d_kernel" % i], shapes["conv_h%d_bias" % i] = (i, d, nh), (nh,)
        names = table_names(L)
        if sorted(variables) != sorted(names):
            raise ValueError("variables must be %s" % ", ".join(names))
        dev = E.require_gpu()
        self.T = {}
        for name in names:
            t = f32(variables[name])
            if t.numel() != int(np.prod(shapes[name])):
                raise ValueError("%s holds %d values, want %s" % (name, t.numel(), "x".join(map(str, shapes[name]))))
            self.T[name] = t.reshape(shapes[name]).contiguous().to(dev)
        self.n_users, self.n_items, self.d, self.L, self.nv, self.nh, self.F = U, I, d, L, nv, nh, F
        self.seq_T, self.neg_samples, self.max_batch = T, N, max_batch
        self.lr, self.l2_reg, self.rate, self.seed = float(lr), float(l2_reg), float(dropout_rate), int(seed)
        self.adam = E.AdamState(lr)
        self.G = {k: torch.zeros_like(t) for k, t in self.T.items()}
        self.m = {k: torch.zeros_like(t) for k, t in self.T.items()}
        self.v = {k: torch.zeros_like(t) for k, t in self.T.items()}
        self._keys = torch.empty(max_batch * (1 + L + T + N), dtype=torch.int64, device=dev)
        floats = C.c_size_t(0)
        call("nrhip_caser_workspace_floats", max_batch, L, d, nv, nh, T, N, C.byref(floats))
        self._ws = torch.empty(max(int(floats.value), 1), dtype=torch.float32, device=dev)
        self._zero_bias = torch.zeros(max(I, 1), dtype=torch.float32, device=dev)
        self.t = 0
        self._seq = None

    def tables(self):
        """{name: tensor} of every variable, in creation order"""
        return dict(self.T)

    @property
    def item_embeddings(self):
        return self.T["item_embeddings"]

    def _fill(self, s, tensors, prefix=""):
        for name, field in FIELDS.items():
            setattr(s, prefix + field, tensors[name].data_ptr())
        for i in range(self.L):
            getattr(s, prefix + "conv_h")[i] = tensors["conv_h%d_kernel" % (i + 1)].data_ptr()
            getattr(s, prefix + "conv_h_bias")[i] = tensors["conv_h%d_bias" % (i + 1)].data_ptr()

    def _weights(self):
        w = CaserWeights()
        self._fill(w, self.T)
        w.n_users, w.n_items, w.d, w.L, w.nv, w.nh = self.n_users, self.n_items, self.d, self.L, self.nv, self.nh
        return w

    # ------------------------------------------------------------------ inputs
    def _check_host(self, name, a, hi, closed):
        """host arrays only: ids in [0, hi) or [0, hi]"""
        if not isinstance(a, torch.Tensor) and np.size(a) and (np.min(a) < 0 or np.max(a) > (hi if closed else hi - 1)):
            raise ValueError("Caser: %s holds an id outside [0, %d%s" % (name, hi, "]" if closed else ")"))

    def _check_feeds(self, users, seq, pos, neg):
        self._check_host("users", users, self.n_users, False)
        self._check_host("seq", seq, self.n_items, True)
        self._check_host("pos", pos, self.n_items, True)
        self._check_host("neg", neg, self.n_items, False)

    def _ids(self, a):
        return as_ids(a, self.T["user_embeddings"].device)

    # ------------------------------------------------------------------ training
    def gradients(self, users, seq, pos, neg, loss_out, mask=None):
        """the C call alone: loss_out (2 floats on the device: loss term, regulariser term) and every gradient; no table
        moves.  Host arrays are checked for ids outside their tables.  An empty batch is no work: nothing is launched
        and loss_out is set to zero."""
        self._check_feeds(users, seq, pos, neg)
        users, seq, pos, neg = self._ids(users), self._ids(seq), self._ids(pos), self._ids(neg)
        B = int(users.shape[0]) if users.dim() == 1 else -1
        if B < 0 or tuple(seq.shape) != (B, self.L) or tuple(pos.shape) != (B, self.seq_T) or \
                tuple(neg.shape) != (B, self.neg_samples):
            raise ValueError("users must be [batch], seq [batch, seq_L], pos [batch, seq_T], neg [batch, neg_samples]")
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if B == 0:
            loss_out.zero_()
            return
        a = CaserStepArgs()
        a.w = self._weights()
        self._fill(a, self.G, "G_")
        a.users, a.seq = _ptr(users, torch.int32), _ptr(seq, torch.int32)
        a.pos, a.neg = _ptr(pos, torch.int32), _ptr(neg, torch.int32)
        if mask is not None:
            if tuple(mask.shape) != (B, self.F):
                raise ValueError("mask must be [batch, nv factors_num + nh seq_L] = (%d, %d)" % (B, self.F))
            a.mask = _ptr(mask, torch.uint8)
        a.keys, a.ws, a.loss2 = _ptr(self._keys), _ptr(self._ws), _ptr(loss_out, torch.float32)
        a.seed, a.batch, a.T, a.N, a.step = self.seed, B, self.seq_T, self.neg_samples, self.t
        a.rate, a.l2_reg = self.rate, self.l2_reg
        call("nrhip_caser_step", C.byref(a), _stream())

    def apply(self):
        """the three gathered tables in Adam's sparse form when there is no regulariser; one dense launch for everything
        else; the gradient buffers are zero again afterwards"""
        dense = []
        for k, t in self.T.items():
            if k in SPARSE_FORM and self.l2_reg == 0.0:
                E.adam_sparse(t, self.m[k], self.v[k], self.G[k], self.adam)
            else:
                dense.append((t, self.m[k], self.v[k], self.G[k], True))
        E.adam_dense_multi(dense, self.adam)
        self.adam.advance()
        self.t += 1

    def step(self, users, seq, pos, neg, loss_out, mask=None):
        """gradients, then Adam; an empty batch moves nothing"""
        self.gradients(users, seq, pos, neg, loss_out, mask)
        if int(np.shape(users)[0]) == 0:
            return
        self.apply()

    def run_schedule(self, users, seq, pos, neg, losses, rows=None, masks=None):
        """a whole epoch: users int32 [S, B], seq [S, B, L], pos [S, B, T], neg [S, B, N], losses float32 [S, 2] on the
        device; host arrays are checked and uploaded once, so there is no host round trip between the steps.  rows [S]:
        the true size of each batch (the last one is filled up), all of B when None.  masks: per step, or None."""
        self._check_feeds(users, seq, pos, neg)
        users, seq, pos, neg = self._ids(users), self._ids(seq), self._ids(pos), self._ids(neg)
        S = int(users.shape[0])
        if users.dim() != 2 or seq.dim() != 3 or pos.dim() != 3 or neg.dim() != 3 or \
                not S == seq.shape[0] == pos.shape[0] == neg.shape[0] or losses.shape[0] < S:
            raise ValueError("users must be [steps, batch], seq, pos and neg [steps, batch, .], losses [steps, 2]")
        for s in range(S):
            n = int(users.shape[1]) if rows is None else int(rows[s])
            self.step(users[s, :n], seq[s, :n], pos[s, :n], neg[s, :n], losses[s], None if masks is None else masks[s])
        return losses

    # ------------------------------------------------------------------ the users' rows and scoring
    def set_sequences(self, seq_ptr, seq):
        """every user's train items in time order: seq[seq_ptr[u]:seq_ptr[u + 1]]"""
        seq_ptr = np.ascontiguousarray(seq_ptr, dtype=np.int64)
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        if seq_ptr.ndim != 1 or len(seq_ptr) < 1 or seq_ptr[0] != 0 or seq_ptr[-1] != len(seq) or \
                (np.diff(seq_ptr) < 0).any():
            raise ValueError("seq_ptr must rise from 0 to len(seq)")
        if len(seq) and (seq.min() < 0 or seq.max() >= self.n_items):
            raise ValueError("Caser: seq holds an item outside [0, %d)" % self.n_items)
        self._seq = (seq_ptr, seq)

    def padded(self, users):
        """[n, L] int32: each user's last L train items, padded in front with I (user_test_seq of Caser.py:156, 168); a
        user without items, or outside the data, is the all-padded row"""
        if self._seq is None:
            raise ValueError("set_sequences() first")
        ptr, seq = self._seq
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        out = np.full((len(users), self.L), self.n_items, np.int32)
        for r, u in enumerate(users):
            if 0 <= u < len(ptr) - 1:
                cut = seq[max(ptr[u], ptr[u + 1] - self.L):ptr[u + 1]]
                if len(cut):
                    out[r, self.L - len(cut):] = cut
        return out

    def forward_rows(self, users, seq):
        """concat(z, user_embeddings[users]) [n, 2d] of the graph with training off, for seq int32 [n, L]"""
        self._check_host("users", users, self.n_users, False)
        self._check_host("seq", seq, self.n_items, True)
        users, seq = self._ids(users), self._ids(seq)
        n = int(users.shape[0]) if users.dim() == 1 else -1
        if n < 0 or tuple(seq.shape) != (n, self.L):
            raise ValueError("users must be [n], seq [n, seq_L]")
        out = torch.empty((n, 2 * self.d), dtype=torch.float32, device=self.T["user_embeddings"].device)
        w = self._weights()
        for lo in range(0, n, self.max_batch):
            pu, ps = users[lo:lo + self.max_batch], seq[lo:lo + self.max_batch]
            call("nrhip_caser_forward", C.byref(w), _ptr(pu, torch.int32), _ptr(ps, torch.int32), int(pu.shape[0]),
                 _ptr(self._ws), C.c_void_p(out[lo:].data_ptr()), 2 * self.d, _stream())
        return out

    def score(self, users):
        """S [n, I] float32 on the device: concat(z, user row) . item_embeddings^T, WITHOUT the item biases
        (Caser.py:122)"""
        users = np.asarray(users, dtype=np.int32).reshape(-1)
        return self.score_rows(users, self.padded(users))

    def score_rows(self, users, seq):
        """score() for padded rows seq int32 [n, L] given as they are"""
        H = self.forward_rows(users, seq)
        n, I = int(H.shape[0]), self.n_items
        out = torch.empty((n, I), dtype=torch.float32, device=H.device)
        h, o = C.c_void_p(H.data_ptr()) if n else None, C.c_void_p(out.data_ptr()) if n and I else None
        if 2 * self.d <= SCORES_MAX_WIDTH:
            call("nrhip_gru4rec_scores", h, 2 * self.d, _ptr(self.T["item_embeddings"]), _ptr(self._zero_bias), n, I,
                 2 * self.d, 0, o, max(I, 1), _stream())
        else:
            call("nrhip_caser_scores", h, 2 * self.d, _ptr(self.T["item_embeddings"]), n, I, 2 * self.d, o, max(I, 1),
                 _stream())
        return out
