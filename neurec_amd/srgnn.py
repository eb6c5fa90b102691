"""SRGNN on the HIP engine: the session graphs and the graph of model/sequential_recommender/SRGNN.py:75-136, one
`sess.run(self.train_opt)` per step, and predict() (csrc/srgnn.hip).

Variables in creation order: nasr_w1, nasr_w2 [d, d], nasrv [1, d], nasr_b [d], embedding [I, d] (read through a concat
with a zero pad row I, which is no row of the table here), W_in [d, d], b_in [d], W_out [d, d], b_out [d], B [2d, d], and
the GRUCell's gates_kernel [3d, 2d], gates_bias [2d], candidate_kernel [3d, d], candidate_bias [d] (made at the cell's
first call, one cell for all `step` iterations, input width 2d).

The loss is the softmax cross-entropy over every item plus L2 * sum v^2 / 2 over ALL 14 variables (the name filter of
SRGNN.py:135 removes nothing).  Every gradient is dense — the table is read through the concat — so every variable
takes ApplyAdam (0.9 / 0.999 / 1e-8).  The learning rate is a per-step input: SRGNN.py:140's staircase decay is the
plugin's `learning_rates`.

The feed is the item ids alone: padded rows [B, L] with targets [B], or (user, end) pairs over the sequences that
`set_sequences` put on the device.  The device builds nodes, alias map and edge lists per session.
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from ._lib import SRGNN_VARS, SrgnnFeed, SrgnnStepArgs, SrgnnWeights, call
from .engine import _ptr, _stream
from .row_learner import ScoreCache, as_ids, f32

MAX_WIDTH = 128               # NRHIP_SRGNN_MAX_WIDTH
MAX_LEN = 256                 # NRHIP_SRGNN_MAX_LEN
MAX_STEP = 4                  # NRHIP_SRGNN_MAX_STEP
MAX_BATCH = 4096              # NRHIP_SRGNN_MAX_BATCH
TABLES = SRGNN_VARS
GUARD = 12345.0               # the value of the guard row behind the table: no kernel may write it


def shapes(I, d):
    return {"nasr_w1": (d, d), "nasr_w2": (d, d), "nasrv": (1, d), "nasr_b": (d,), "embedding": (I, d), "W_in": (d, d),
            "b_in": (d,), "W_out": (d, d), "b_out": (d,), "B": (2 * d, d), "gates_kernel": (3 * d, 2 * d),
            "gates_bias": (2 * d,), "candidate_kernel": (3 * d, d), "candidate_bias": (d,)}


def _limit(name, value, hi):
    if not 1 <= value <= hi:
        raise NotImplementedError("SRGNN: %s=%d is not supported (1 to %d)" % (name, value, hi))


class SRGNNEngine:
    """Tables, optimiser slots and gradient buffers in HBM.

    `variables`: {name: array} of TABLES.  `step(seq, target, loss_out, lr=None)`: one batch — seq int32 [B, L]
    post-padded with I, target [B] — gradients, then Adam at learning rate lr.  `run_schedule(users, ends, losses, lrs)`
    issues an epoch from the resident sequences.  `forward_rows(seq)` -> the session embeddings [n, d]; `score(users)`
    -> [n, I] on the device."""

    def __init__(self, variables, lr, L2, max_batch, max_seq_len, step, nonhybrid=False):
        emb = f32(variables["embedding"])
        if emb.dim() != 2:
            raise ValueError("embedding must be [num_items, hidden_size]")
        I, d = int(emb.shape[0]), int(emb.shape[1])
        L, S, max_batch = int(max_seq_len), int(step), int(max_batch)
        _limit("hidden_size", d, MAX_WIDTH)
        _limit("max_seq_len", L, MAX_LEN)
        _limit("step", S, MAX_STEP)
        _limit("batch_size", max_batch, MAX_BATCH)
        if max_batch * I >= 1 << 31:
            raise NotImplementedError("SRGNN: batch_size * num_items = %d is not supported (below 2^31)" % (max_batch * I))
        if I < 1:
            raise ValueError("SRGNN: no items")
        if sorted(variables) != sorted(TABLES):
            raise ValueError("variables must be %s" % ", ".join(TABLES))
        dev = E.require_gpu()
        want = shapes(I, d)
        self.T = {}
        for name in TABLES:
            t = f32(variables[name])
            if t.numel() != int(np.prod(want[name])):
                raise ValueError("%s holds %d values, want %s" % (name, t.numel(), "x".join(map(str, want[name]))))
            t = t.reshape(want[name]).contiguous()
            if name == "embedding":                  # a guard row behind the table, where the reference has its pad row
                self._store = torch.full((I + 1, d), GUARD, dtype=torch.float32, device=dev)
                self._store[:I] = t.to(dev)
                self.T[name] = self._store[:I]
            else:
                self.T[name] = t.to(dev)
        self.n_items, self.d, self.L, self.S, self.max_batch = I, d, L, S, max_batch
        self.nonhybrid, self.L2 = bool(nonhybrid), float(L2)
        self.adam = E.AdamState(lr)
        self.G = {k: torch.zeros_like(t) for k, t in self.T.items()}
        self.m = {k: torch.zeros_like(t) for k, t in self.T.items()}
        self.v = {k: torch.zeros_like(t) for k, t in self.T.items()}
        self._keys = torch.empty(max_batch * L, dtype=torch.int64, device=dev)
        floats = C.c_size_t(0)
        call("nrhip_srgnn_workspace_floats", max_batch, L, d, S, I, C.byref(floats))
        self._ws = torch.empty(max(int(floats.value), 1), dtype=torch.float32, device=dev)
        self._scores = ScoreCache()
        self._seq = None
        self.forward_calls = 0

    def tables(self):
        """{name: tensor} of every variable, in creation order"""
        return dict(self.T)

    @property
    def guard_row(self):
        return self._store[self.n_items]

    def _weights(self):
        w = SrgnnWeights()
        for name in TABLES:
            setattr(w, name, self.T[name].data_ptr())
        w.n_items, w.d, w.L, w.step, w.nonhybrid = self.n_items, self.d, self.L, self.S, int(self.nonhybrid)
        return w

    # ------------------------------------------------------------------ inputs
    def _dev(self):
        return self.T["embedding"].device

    def _check_host(self, name, a, hi, closed):
        """host arrays only: ids in [0, hi) or [0, hi]"""
        if not isinstance(a, torch.Tensor) and np.size(a) and (np.min(a) < 0 or np.max(a) > (hi if closed else hi - 1)):
            raise ValueError("SRGNN: %s holds an id outside [0, %d%s" % (name, hi, "]" if closed else ")"))

    def _rows_feed(self, seq, target):
        """(feed, batch, the tensors it points into) of padded rows"""
        self._check_host("seq", seq, self.n_items, True)
        seq = as_ids(seq, self._dev())
        if seq.dim() != 2 or seq.shape[1] != self.L:
            raise ValueError("seq must be [batch, max_seq_len]")
        f = SrgnnFeed()
        f.seq = _ptr(seq, torch.int32)
        if target is not None:
            self._check_host("target", target, self.n_items, False)
            target = as_ids(target, self._dev())
            if tuple(target.shape) != (int(seq.shape[0]),):
                raise ValueError("target must be [batch]")
            f.target = _ptr(target, torch.int32)
        return f, int(seq.shape[0]), (seq, target)

    def _pairs_feed(self, users, ends):
        """(feed, batch, the tensors it points into) of (user, end) pairs over the resident sequences"""
        if self._seq is None:
            raise ValueError("set_sequences() first")
        ptr, flat, counts = self._seq
        if not isinstance(users, torch.Tensor):
            users, ends = np.asarray(users), np.asarray(ends)
            self._check_host("users", users, len(counts), False)
            if users.shape != ends.shape or (users.size and ((ends < 0).any() or (ends > counts[users]).any())):
                raise ValueError("SRGNN: an end outside its user's sequence")
        users, ends = as_ids(users, self._dev()), as_ids(ends, self._dev())
        if users.dim() != 1 or users.shape != ends.shape:
            raise ValueError("users and ends must be [batch]")
        f = SrgnnFeed()
        f.users, f.ends = _ptr(users, torch.int32), _ptr(ends, torch.int32)
        f.seq_ptr, f.seq_flat, f.n_users = _ptr(ptr, torch.int64), _ptr(flat, torch.int32), len(counts)
        return f, int(users.shape[0]), (users, ends)

    # ------------------------------------------------------------------ training
    def _gradients(self, feed, B, loss_out):
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if B == 0:
            loss_out.zero_()
            return
        a = SrgnnStepArgs()
        a.w, a.f = self._weights(), feed
        for name in TABLES:
            setattr(a, "G_" + name, self.G[name].data_ptr())
        a.keys, a.ws, a.loss2 = _ptr(self._keys), _ptr(self._ws), _ptr(loss_out, torch.float32)
        a.batch, a.l2 = B, self.L2
        call("nrhip_srgnn_step", C.byref(a), _stream())

    def gradients(self, seq, target, loss_out):
        """the C call alone: loss_out (2 floats on the device: cross-entropy mean, regulariser term) and every gradient;
        no table moves.  Host arrays are checked for ids outside the table.  An empty batch launches nothing."""
        feed, B, keep = self._rows_feed(seq, target)
        if target is None:
            raise ValueError("a step needs targets")
        self._gradients(feed, B, loss_out)
        return B

    def apply(self, lr=None):
        """ApplyAdam on every variable in one launch; the gradient buffers are zero again afterwards"""
        if lr is not None:
            self.adam.lr = np.float32(lr)
        E.adam_dense_multi([(t, self.m[k], self.v[k], self.G[k], True) for k, t in self.T.items()], self.adam)
        self.adam.advance()

    def step(self, seq, target, loss_out, lr=None):
        """gradients, then Adam at learning rate lr (the engine's own when None); an empty batch moves nothing"""
        if self.gradients(seq, target, loss_out):
            self.apply(lr)

    def run_schedule(self, users, ends, losses, lrs=None):
        """a whole epoch from the resident sequences: users, ends int32 [S, B] — session = the last max_seq_len of the
        user's first `end` items, target = the item at `end` — losses float32 [S, 2] on the device, lrs [S] the step's
        learning rates.  The pairs are checked and uploaded once; no [S, B, L] array exists anywhere."""
        if self._seq is None:
            raise ValueError("set_sequences() first")
        counts = self._seq[2]
        if not isinstance(users, torch.Tensor):
            users, ends = np.asarray(users), np.asarray(ends)
            self._check_host("users", users, len(counts), False)
            if users.shape != ends.shape or (users.size and ((ends < 0).any() or (ends >= counts[users]).any())):
                raise ValueError("SRGNN: an end without a target in its user's sequence")
        users, ends = as_ids(users, self._dev()), as_ids(ends, self._dev())
        if users.dim() != 2 or users.shape != ends.shape or losses.shape[0] < users.shape[0]:
            raise ValueError("users and ends must be [steps, batch], losses [steps, 2]")
        for s in range(int(users.shape[0])):
            feed, B, keep = self._pairs_feed(users[s], ends[s])
            self._gradients(feed, B, losses[s])
            if B:
                self.apply(None if lrs is None else lrs[s])
        return losses

    # ------------------------------------------------------------------ the sessions' rows and scoring
    def set_sequences(self, seq_ptr, seq):
        """every user's train items in time order, on the device: seq[seq_ptr[u]:seq_ptr[u + 1]]"""
        seq_ptr = np.ascontiguousarray(seq_ptr, dtype=np.int64)
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        if seq_ptr.ndim != 1 or len(seq_ptr) < 1 or seq_ptr[0] != 0 or seq_ptr[-1] != len(seq) or \
                (np.diff(seq_ptr) < 0).any():
            raise ValueError("seq_ptr must rise from 0 to len(seq)")
        if len(seq) and (seq.min() < 0 or seq.max() >= self.n_items):
            raise ValueError("SRGNN: seq holds an item outside [0, %d)" % self.n_items)
        dev = self._dev()
        flat = torch.from_numpy(seq if len(seq) else np.zeros(1, np.int32)).to(dev)
        self._seq = (torch.from_numpy(seq_ptr).to(dev), flat, np.diff(seq_ptr))

    def _forward(self, make_feed, n):
        out = torch.empty((n, self.d), dtype=torch.float32, device=self._dev())
        w = self._weights()
        for lo in range(0, n, self.max_batch):
            feed, rows, keep = make_feed(lo, min(lo + self.max_batch, n))
            call("nrhip_srgnn_forward", C.byref(w), C.byref(feed), rows, _ptr(self._ws), C.c_void_p(out[lo:].data_ptr()),
                 self.d, _stream())
            self.forward_calls += 1
        return out

    def forward_rows(self, seq):
        """the session embeddings [n, d] of padded rows seq int32 [n, L]"""
        self._check_host("seq", seq, self.n_items, True)
        seq = as_ids(seq, self._dev())
        if seq.dim() != 2 or seq.shape[1] != self.L:
            raise ValueError("seq must be [n, max_seq_len]")
        return self._forward(lambda lo, hi: self._rows_feed(seq[lo:hi], None), int(seq.shape[0]))

    def forward_users(self, users):
        """the session embeddings [n, d] of the users' last max_seq_len train items; a user without items, or outside
        the data, has the empty session: a zero row"""
        if self._seq is None:
            raise ValueError("set_sequences() first")
        counts = self._seq[2]
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        inside = (users >= 0) & (users < len(counts))
        ends = np.where(inside, counts[np.where(inside, users, 0)] if len(counts) else 0, 0).astype(np.int32)
        users = np.where(inside, users, 0).astype(np.int32)
        return self._forward(lambda lo, hi: self._pairs_feed(users[lo:hi], ends[lo:hi]), len(users))

    def score(self, users):
        """S [n, I] float32 on the device: sess . embedding^T (SRGNN.py:130)"""
        return self._scores.score(self.forward_users(users), self.T["embedding"], self.n_items)
