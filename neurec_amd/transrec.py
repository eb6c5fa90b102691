"""TransRec on the HIP engine: the graph of model/sequential_recommender/TransRec.py:66-107 and one
`sess.run((loss, optimizer))` per step, and predict() (csrc/transrec.hip).

An instance is (user, recent item, item[, negative]), v = P_u + T + Q_l - Q_i, and its training score the SQUARED
distance x = b_i - |v|^2; predict() ranks by b_j - |P_u + T + Q_last(u) - Q_j|, the distance itself.  One item table Q
is read as the recent item, as the target and as the negative in the same batch.

Optimiser forms, as TF-1.12 picks them: P, Q and b are read through embedding_lookup only — the sparse application
(neurec_amd/row_learner.py), b as a [num_items, 1] table; T is read through tf.tile — the dense Apply* kernels, every
step.

The score has no factor form: evaluation has a kernel of its own, the direct-difference distance.
"""
import ctypes as C

import torch

from . import engine as E
from ._lib import TransrecStepArgs, call
from .engine import _ptr, _stream
from .row_learner import RowLearner, addr, as_ids, check_loss_learner, f32

MAX_D = 128                   # NRHIP_TRANSREC_MAX_D
GT_CHUNK = 32                 # NRHIP_TRANSREC_CHUNK: instances per partial sum of G_T
GT_MAX_CHUNKS = 64            # NRHIP_TRANSREC_MAX_CHUNKS
_ROWS = ("P", "Q", "b")
_TABLES = _ROWS + ("T",)


class TransRecEngine:
    """Tables P [U, d], Q [I, d], b [I], T [d], their optimiser state and gradient buffers in HBM.

    `step(users, recent, items, third, loss_out)`: one batch of the time-order instance stream at high_order = 1 —
    pointwise (third = float labels) or pairwise (third = int32 negatives).  `score(users, last_items)` -> [n, I] on
    the device."""

    def __init__(self, P, Q, b, T, lr, reg_mf, max_batch, loss="bpr", pairwise=True, learner="adam", momentum=0.9):
        loss, learner, self.loss_kind = check_loss_learner(loss, learner, pairwise)
        P, Q, b, T = f32(P), f32(Q), f32(b).reshape(-1), f32(T).reshape(-1)
        if P.dim() != 2 or Q.dim() != 2 or Q.shape[1] != P.shape[1]:
            raise ValueError("P must be [num_users, embedding_size], Q [num_items, embedding_size]")
        (U, d), I = P.shape, Q.shape[0]
        if d < 1 or d > MAX_D:
            raise NotImplementedError("TransRec: embedding_size=%d is not supported (1 to %d)" % (d, MAX_D))
        if b.numel() != I or T.numel() != d:
            raise ValueError("b must hold num_items entries and T embedding_size entries")
        dev = E.require_gpu()
        self.loss, self.pairwise, self.learner = loss, bool(pairwise), learner
        self.n_users, self.n_items, self.d = U, I, d
        self.P, self.Q, self.b, self.T = (t.contiguous().to(dev) for t in (P, Q, b, T))
        self.G = {k: torch.zeros_like(getattr(self, k)) for k in _TABLES}
        self.lr, self.momentum, self.reg_mf = float(lr), float(momentum), float(reg_mf)
        self.adam = E.AdamState(lr)
        self.opt = RowLearner(learner, lr, momentum, self.adam)
        self.dense = self.opt.dense                           # T; None: ApplyAdam
        slots = {k: self.opt.slots(getattr(self, k)) for k in _TABLES}
        self.s0, self.s1 = ({k: s[i] for k, s in slots.items()} for i in (0, 1))
        self.flag = {k: self.opt.flag(getattr(self, k).shape[0], dev) for k in _ROWS}
        self.max_batch = int(max_batch)
        mb = max(self.max_batch, 1)
        self._keys = torch.empty(3 * mb * (2 if self.pairwise else 1), dtype=torch.int64, device=dev)
        self._scal = torch.empty(4 * mb, dtype=torch.float32, device=dev)
        self._partial = torch.empty((min((mb + GT_CHUNK - 1) // GT_CHUNK, GT_MAX_CHUNKS), d), dtype=torch.float32,
                                    device=dev)
        self.t = 0

    # ------------------------------------------------------------------ training
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
            setattr(a, "flag_" + k, addr(self.flag[k]))
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
            self.opt.apply(getattr(self, k), self.s0[k], self.s1[k], self.G[k], self.flag[k])
        self.opt.apply_dense([(self.T, self.s0["T"], self.s1["T"], self.G["T"])], clear_grad=True)
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
    def queries(self, last_items, users=None):
        """[n, d] rows P_u + T + Q_last(u) of `users` (None: every user); last -1: P_u + T"""
        dev = self.P.device
        users = None if users is None else as_ids(users, dev)
        last = as_ids(last_items, dev, self.n_users, "last_items holds {n} entries, the user table {want} rows")
        n = self.n_users if users is None else int(users.numel())
        out = torch.empty((n, self.d), dtype=torch.float32, device=dev)
        call("nrhip_transrec_queries", _ptr(self.P), _ptr(self.Q), _ptr(self.T), self.n_users, self.n_items, self.d,
             _ptr(last, torch.int32), _ptr(users, torch.int32, allow_none=True), n, _ptr(out),
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
