"""TransRec on the HIP engine: the graph of model/sequential_recommender/TransRec.py:66-107 and one
`sess.run((loss, optimizer))` per step, and predict() (csrc/transrec.hip).

An instance is (user, recent item, item[, negative]), v = P_u + T + Q_l - Q_i, and its training score the SQUARED
distance x = b_i - |v|^2; predict() ranks by b_j - |P_u + T + Q_last(u) - Q_j|, the distance itself.  One item table Q
is read as the recent item, as the target and as the negative in the same batch.

Optimiser forms, as TF-1.12 picks them: P, Q and b are read through embedding_lookup only — the sparse application
(Adam's sparse form, every row swept; the row kernels for gd / adagrad / rmsprop / momentum), b as HistoryEngine's
`bias`; T is read through tf.tile — the dense Apply* kernels, every step.

The score has no factor form: evaluation has a kernel of its own, the direct-difference distance.
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from ._lib import TransrecStepArgs, call
from .engine import _ptr, _stream

MAX_D = 128                   # NRHIP_TRANSREC_MAX_D
GT_CHUNK = 32                 # NRHIP_TRANSREC_CHUNK: instances per partial sum of G_T
GT_MAX_CHUNKS = 64            # NRHIP_TRANSREC_MAX_CHUNKS
_ROWS = ("P", "Q", "b")
_TABLES = _ROWS + ("T",)


def _addr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32)


class TransRecEngine:
    """Tables P [U, d], Q [I, d], b [I], T [d], their optimiser state and gradient buffers in HBM.

    `step(users, recent, items, third, loss_out)`: one batch of the time-order instance stream at high_order = 1 —
    pointwise (third = float labels) or pairwise (third = int32 negatives).  `score(users, last_items)` -> [n, I] on
    the device."""

    def __init__(self, P, Q, b, T, lr, reg_mf, max_batch, loss="bpr", pairwise=True, learner="adam", momentum=0.9):
        loss, learner = str(loss).lower(), str(learner).lower()
        table = E.PAIRWISE_LOSSES if pairwise else E.POINTWISE_LOSSES
        if loss not in table:
            raise Exception("please choose a suitable loss function")        # learner.py:28,40
        if learner != "adam" and learner not in E.ROW_OPTIMIZERS:
            raise ValueError("please select a suitable optimizer")           # learner.py:15
        P, Q, b, T = _f32(P), _f32(Q), _f32(b).reshape(-1), _f32(T).reshape(-1)
        if P.dim() != 2 or Q.dim() != 2 or Q.shape[1] != P.shape[1]:
            raise ValueError("P must be [num_users, embedding_size], Q [num_items, embedding_size]")
        (U, d), I = P.shape, Q.shape[0]
        if d < 1 or d > MAX_D:
            raise NotImplementedError("TransRec: embedding_size=%d is not supported (1 to %d)" % (d, MAX_D))
        if b.numel() != I or T.numel() != d:
            raise ValueError("b must hold num_items entries and T embedding_size entries")
        dev = E.require_gpu()
        self.loss, self.pairwise, self.learner = loss, bool(pairwise), learner
        self.loss_kind = table[loss]
        self.n_users, self.n_items, self.d = U, I, d
        self.P, self.Q, self.b, self.T = (t.contiguous().to(dev) for t in (P, Q, b, T))
        self.G = {k: torch.zeros_like(getattr(self, k)) for k in _TABLES}
        self.lr, self.momentum, self.reg_mf = float(lr), float(momentum), float(reg_mf)
        self.adam = E.AdamState(lr)
        self.dense = E.make_learner(learner, lr)               # T; None: ApplyAdam
        if self.dense is not None:
            self.dense.momentum = self.momentum
        init = {"adam": 0.0, "gd": None, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        two = learner in ("adam", "rmsprop")
        mk = lambda t, v: None if v is None else torch.full_like(t, v)
        self.s0 = {k: mk(getattr(self, k), init) for k in _TABLES}
        self.s1 = {k: (mk(getattr(self, k), 0.0) if two else None) for k in _TABLES}
        rows = learner != "adam"
        self.flag = {k: (torch.zeros(getattr(self, k).shape[0], dtype=torch.uint8, device=dev) if rows else None)
                     for k in _ROWS}
        self.max_batch = int(max_batch)
        mb = max(self.max_batch, 1)
        self._keys = torch.empty(3 * mb * (2 if self.pairwise else 1), dtype=torch.int64, device=dev)
        self._scal = torch.empty(4 * mb, dtype=torch.float32, device=dev)
        self._partial = torch.empty((min((mb + GT_CHUNK - 1) // GT_CHUNK, GT_MAX_CHUNKS), d), dtype=torch.float32,
                                    device=dev)
        self.t = 0

    # ------------------------------------------------------------------ training
    def _apply_rows(self, key):
        var, grad, s0, s1, flag = getattr(self, key), self.G[key], self.s0[key], self.s1[key], self.flag[key]
        rows = var.shape[0]
        v2 = lambda s: None if s is None else s.view(rows, -1)
        if self.learner == "adam":
            E.adam_sparse(var, s0, s1, grad, self.adam)
        elif self.learner == "rmsprop":
            E.optimizer_rows("rmsprop", v2(var), v2(s0), v2(s1), v2(grad), flag, self.lr, 0.9, 0.0, 1e-10)
        elif self.learner == "momentum":
            E.optimizer_rows("momentum", v2(var), v2(s0), None, v2(grad), flag, self.lr, self.momentum)
        else:
            E.optimizer_rows(self.learner, v2(var), v2(s0), None, v2(grad), flag, self.lr)

    def _apply_dense(self):
        if self.dense is None:
            E.adam_dense(self.T, self.s0["T"], self.s1["T"], self.G["T"], self.adam, clear_grad=True)
        else:
            self.dense.apply([(self.T, self.s0["T"], self.s1["T"], self.G["T"], True)])

    def gradients(self, users, recent, items, third, loss_out):
        """the C call alone: loss_out, the batch's rows of G_P / G_Q / G_b (and the row flags) and G_T whole; no table
        moves.  An empty batch is no work: nothing is launched and loss_out is set to zero."""
        B = int(users.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if recent.numel() != B or items.numel() != B or third.numel() != B:
            raise ValueError("users, recent items, items and the fourth field must have the same length")
        if B == 0:
            loss_out.zero_()
            return
        a = TransrecStepArgs()
        for k in _TABLES:
            setattr(a, k, _ptr(getattr(self, k)))
            setattr(a, "G_" + k, _ptr(self.G[k]))
        for k in _ROWS:
            setattr(a, "flag_" + k, _addr(self.flag[k]))
        a.users, a.recent, a.items = _ptr(users, torch.int32), _ptr(recent, torch.int32), _ptr(items, torch.int32)
        a.third = _ptr(third, torch.int32 if self.pairwise else torch.float32)
        a.keys, a.scal, a.partial = _ptr(self._keys), _ptr(self._scal), _ptr(self._partial)
        a.loss2 = _ptr(loss_out, torch.float32)
        a.n_users, a.n_items, a.d, a.batch = self.n_users, self.n_items, self.d, B
        a.pairwise, a.loss_kind, a.reg = int(self.pairwise), self.loss_kind, self.reg_mf
        call("nrhip_transrec_step", C.byref(a), _stream())

    def apply(self):
        """three sparse applications and the dense one of T; the gradient buffers (and flags) are zero again
        afterwards"""
        for k in _ROWS:
            self._apply_rows(k)
        self._apply_dense()
        self.adam.advance()
        self.t += 1

    def step(self, users, recent, items, third, loss_out):
        """pointwise: third = labels (float32); pairwise: third = negative items (int32).  loss_out: 2 floats on the
        device, (loss term, regulariser term) of the batch before the update.  An empty batch moves nothing, the step
        counter included."""
        self.gradients(users, recent, items, third, loss_out)
        if int(users.numel()):
            self.apply()

    # ------------------------------------------------------------------ scoring
    def _last(self, last_items):
        if not isinstance(last_items, torch.Tensor):
            last_items = torch.from_numpy(np.ascontiguousarray(last_items, dtype=np.int32))
        last_items = last_items.to(self.P.device, torch.int32).contiguous()
        if last_items.numel() != self.n_users:
            raise ValueError("last_items holds %d entries, the user table %d rows" % (last_items.numel(), self.n_users))
        return last_items

    def _users(self, users):
        if users is None:
            return None
        if not isinstance(users, torch.Tensor):
            users = torch.from_numpy(np.ascontiguousarray(users, dtype=np.int32))
        return users.to(self.P.device, torch.int32).contiguous()

    def queries(self, last_items, users=None):
        """[n, d] rows P_u + T + Q_last(u) of `users` (None: every user); last -1: P_u + T"""
        users = self._users(users)
        n = self.n_users if users is None else int(users.numel())
        out = torch.empty((n, self.d), dtype=torch.float32, device=self.P.device)
        call("nrhip_transrec_queries", _ptr(self.P), _ptr(self.Q), _ptr(self.T), self.n_users, self.n_items, self.d,
             _ptr(self._last(last_items), torch.int32), _ptr(users, torch.int32, allow_none=True), n, _ptr(out),
             out.stride(0), _stream())
        return out

    def score_queries(self, q, out=None):
        """S [n, I]: b_j - |q_r - Q_j| for the query rows q [n, d]; `out` may be a [n, >= I] buffer whose first I columns
        are written"""
        n, I = int(q.shape[0]), self.n_items
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError("queries must be [n, embedding_size]")
        if out is None:
            out = torch.empty((n, I), dtype=torch.float32, device=self.P.device)
        elif out.dim() != 2 or out.shape[0] != n or out.shape[1] < I or out.stride(1) != 1:
            raise ValueError("out must be [n, >= num_items] with unit column stride")
        call("nrhip_transrec_scores", C.c_void_p(q.data_ptr()) if n else None, q.stride(0) if n else self.d,
             _ptr(self.Q), _ptr(self.b), n, I, self.d, C.c_void_p(out.data_ptr()) if n and I else None,
             out.stride(0) if n else max(I, 1), _stream())
        return out

    def score(self, users, last_items):
        """S [n, I] float32 on the device: TransRec.py:153-161 for `users`, every item, own items included"""
        return self.score_queries(self.queries(last_items, users))
