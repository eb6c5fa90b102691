"""NPE on the HIP engine: the graph of model/sequential_recommender/NPE.py:54-75 and one
`sess.run((loss, optimizer))` per step (csrc/npe.hip).

An instance is (user, recents r_0..r_{L-1}, item, label): s = the sum of the W rows of the recents,
q = relu(P[u]) + relu(s), x = <relu(V[i]), q>.  The three tables are read through embedding_lookup only, so TF-1.12
gives all three the sparse application (neurec_amd/row_learner.py).

The score is a factor form of width d, x(u, i) = <h_u, relu(V[i])> with h_u = relu(P[u]) + relu(sum of W over the
user's last items) (`last_items`, int32 [U, L], -1 = a slot that takes no part): evaluation is the factor path, its
item side the transformed table relu(V), which the library writes into a buffer of its own.
"""
import ctypes as C

import torch

from . import engine as E
from ._lib import NpeStepArgs, call
from .engine import _ptr, _stream
from .row_learner import RowLearner, ScoreCache, addr, as_ids, check_loss_learner, f32

MAX_D = 128                   # NRHIP_NPE_MAX_D
MAX_ORDER = 16                # NRHIP_NPE_MAX_ORDER
_TABLES = ("P", "V", "W")


class NPEEngine:
    """Tables P [U, d], V [I, d] and W [I, d], their optimiser state and gradient buffers in HBM.

    `step(users, recents, items, labels, loss_out)`: one batch of the time-order pointwise stream at high_order = L,
    recents int32 [B, L], oldest first (the context sum is taken in that order).  `score(users)` -> [n, I] on the
    device."""

    def __init__(self, P, V, W, lr, reg, max_batch, high_order, loss="cross_entropy", learner="adam", momentum=0.9,
                 last_items=None):
        loss, learner, self.loss_kind = check_loss_learner(loss, learner, pairwise=False)
        P, V, W = f32(P), f32(V), f32(W)
        if P.dim() != 2 or V.dim() != 2 or V.shape[1] != P.shape[1] or W.shape != V.shape:
            raise ValueError("P must be [num_users, embedding_size], V and W [num_items, embedding_size]")
        (U, d), I, L = P.shape, V.shape[0], int(high_order)
        if d < 1 or d > MAX_D:
            raise NotImplementedError("NPE: embedding_size=%d is not supported (1 to %d)" % (d, MAX_D))
        if L < 1 or L > MAX_ORDER:
            raise NotImplementedError("NPE: high_order=%d is not supported (1 to %d)" % (L, MAX_ORDER))
        dev = E.require_gpu()
        self.loss, self.learner = loss, learner
        self.n_users, self.n_items, self.d, self.L = U, I, d, L
        self.P, self.V, self.W = (t.contiguous().to(dev) for t in (P, V, W))
        self.G = {k: torch.zeros_like(getattr(self, k)) for k in _TABLES}
        self.lr, self.momentum, self.reg = float(lr), float(momentum), float(reg)
        self.adam = E.AdamState(lr)
        self.opt = RowLearner(learner, lr, momentum, self.adam)
        slots = {k: self.opt.slots(getattr(self, k)) for k in _TABLES}
        self.s0, self.s1 = ({k: s[i] for k, s in slots.items()} for i in (0, 1))
        self.flag = {k: self.opt.flag(getattr(self, k).shape[0], dev) for k in _TABLES}
        self.max_batch = int(max_batch)
        N = max(self.max_batch, 1)
        self._keys = torch.empty((2 + L) * N, dtype=torch.int64, device=dev)
        self._scal = torch.empty(4 * N, dtype=torch.float32, device=dev)
        self._s = torch.empty((N, d), dtype=torch.float32, device=dev)       # the context sums
        self._ds = torch.empty((N, d), dtype=torch.float32, device=dev)      # their derivative, already gated
        self.t = 0
        self.last_items = None if last_items is None else self._last(last_items)
        self._factors = None                                   # (step, h_u of every user)
        self._q = None                                         # (step, relu(V))
        self._scores = ScoreCache()

    def gradients(self, users, recents, items, labels, loss_out):
        """the C call alone: loss_out and the batch's rows of self.G (and the row flags); no table moves"""
        B = int(users.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if items.numel() != B or labels.numel() != B:
            raise ValueError("users, items and labels must have the same length")
        if recents.numel() != B * self.L:
            raise ValueError("recents must hold high_order = %d entries per slot" % self.L)
        if B == 0:                                     # the C call wants addresses: any buffer does, nothing is read
            users = recents = items = self._keys.view(torch.int32)
            labels = self._scal
        a = NpeStepArgs()
        for k in _TABLES:
            setattr(a, k, _ptr(getattr(self, k)))
            setattr(a, "G_" + k, _ptr(self.G[k]))
            setattr(a, "flag_" + k, addr(self.flag[k]))
        a.users, a.recents, a.items = _ptr(users, torch.int32), _ptr(recents, torch.int32), _ptr(items, torch.int32)
        a.labels = _ptr(labels, torch.float32)
        a.keys, a.scal, a.loss2 = _ptr(self._keys), _ptr(self._scal), _ptr(loss_out, torch.float32)
        a.s, a.ds = _ptr(self._s), _ptr(self._ds)
        a.n_users, a.n_items, a.d, a.L, a.batch = self.n_users, self.n_items, self.d, self.L, B
        a.loss_kind, a.reg = self.loss_kind, self.reg
        call("nrhip_npe_step", C.byref(a), _stream())

    def apply(self):
        """the three applications of self.G; the gradient rows (and flags) are zero again afterwards"""
        for k in _TABLES:
            self.opt.apply(getattr(self, k), self.s0[k], self.s1[k], self.G[k], self.flag[k])
        self.adam.advance()
        self.t += 1

    def step(self, users, recents, items, labels, loss_out):
        """recents: int32 [B, L] (or [B] when L = 1); labels float32.  loss_out: 2 floats on the device, (loss term,
        regulariser term) of the batch before the update."""
        self.gradients(users, recents, items, labels, loss_out)
        self.apply()

    # ------------------------------------------------------------------ scoring
    def _last(self, last_items):
        return as_ids(last_items, self.P.device, self.n_users * self.L,
                      "last_items holds {n} entries, not [num_users, high_order] = [%d, %d]" % (self.n_users, self.L))

    def _need_last(self, last_items):
        if last_items is None:
            if self.last_items is None:
                raise ValueError("scoring needs the [num_users, high_order] table of last items")
            return self.last_items
        return self._last(last_items)

    def user_factors(self, users=None, last_items=None):
        """[n, d] rows h_u = relu(P[u]) + relu(sum of W over last_items[u]) of `users` (int32 device tensor; None:
        every user; last_items None: the table the engine was built with); a user with no entry there gets
        h_u = relu(P[u])"""
        last = self._need_last(last_items)
        n = self.n_users if users is None else int(users.numel())
        out = torch.empty((n, self.d), dtype=torch.float32, device=self.P.device)
        call("nrhip_npe_user_factors", _ptr(self.P), _ptr(self.W), self.n_users, self.n_items, self.d, self.L,
             _ptr(last, torch.int32), _ptr(users, torch.int32, allow_none=True), n, _ptr(out),
             out.stride(0) if n else self.d, _stream())
        return out

    def item_factors(self):
        """[I, d]: relu(V), written by the library into a buffer of its own"""
        out = torch.empty_like(self.V)
        call("nrhip_npe_item_factors", _ptr(self.V), self.n_items, self.d, _ptr(out), _stream())
        return out

    def _item_side(self):
        """relu(V) as of this step: rebuilt only after a step"""
        q = self._q
        if q is None or q[0] != self.t:
            self._q = q = (self.t, self.item_factors())
        return q[1]

    def eval_factors(self):
        """(h [U, d], relu(V) [I, d]) whose inner products are predict()'s rows; both are rebuilt only after a step"""
        f = self._factors
        if f is None or f[0] != self.t:
            self._factors = (self.t, self.user_factors())
        return self._factors[1], self._item_side()

    def score(self, users, last_items=None):
        """S [n, I] float32 on the device: NPE.py:114-142 for `users`, every item, own items included"""
        H = self.user_factors(as_ids(users, self.P.device), last_items)
        return self._scores.score(H, self._item_side(), self.n_items)
