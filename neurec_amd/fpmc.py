"""FPMC on the HIP engine: the graph of model/sequential_recommender/FPMC.py:61-88 and one
`sess.run((loss, optimizer))` per step (csrc/fpmc.hip).

An instance is (user, recent item, item[, negative]) and its score x(u, l, i) = <UI[u], IU[i]> + <IL[i], LI[l]>.  All
four tables are read through embedding_lookup only, so TF-1.12 gives every one the sparse application
(neurec_amd/row_learner.py).

The score has a factor form, x(u, l, i) = [UI[u] | LI[l]] . [IU[i] | IL[i]]: evaluation is the factor path at width
2 d with l = the user's most recent train item.
"""
import ctypes as C

import torch

from . import engine as E
from ._lib import FpmcStepArgs, call
from .engine import _ptr, _stream
from .row_learner import RowLearner, ScoreCache, addr, as_ids, check_loss_learner, f32

MAX_D = 128                   # NRHIP_FPMC_MAX_D
_TABLES = ("UI", "IU", "IL", "LI")


class FPMCEngine:
    """Tables UI [U, d], IU / IL / LI [I, d], their optimiser state and gradient buffers in HBM.

    `step(users, recent, items, third, loss_out)`: one batch of the time-order instance stream at high_order = 1 —
    pointwise (third = float labels) or pairwise (third = int32 negatives).  `score(users, last_items)` -> [n, I] on
    the device."""

    def __init__(self, UI, IU, IL, LI, lr, reg_mf, max_batch, loss="cross_entropy", pairwise=False, learner="adam",
                 momentum=0.9):
        loss, learner, self.loss_kind = check_loss_learner(loss, learner, pairwise)
        UI, IU, IL, LI = f32(UI), f32(IU), f32(IL), f32(LI)
        if UI.dim() != 2 or IU.dim() != 2 or IU.shape[1] != UI.shape[1] or \
                tuple(IL.shape) != tuple(IU.shape) or tuple(LI.shape) != tuple(IU.shape):
            raise ValueError("UI must be [num_users, embedding_size], IU / IL / LI [num_items, embedding_size]")
        (U, d), I = UI.shape, IU.shape[0]
        if d < 1 or d > MAX_D:
            raise NotImplementedError("FPMC: embedding_size=%d is not supported (1 to %d)" % (d, MAX_D))
        dev = E.require_gpu()
        self.loss, self.pairwise, self.learner = loss, bool(pairwise), learner
        self.n_users, self.n_items, self.d = U, I, d
        self.UI, self.IU, self.IL, self.LI = (t.contiguous().to(dev) for t in (UI, IU, IL, LI))
        self.G = {k: torch.zeros_like(getattr(self, k)) for k in _TABLES}
        self.lr, self.momentum, self.reg_mf = float(lr), float(momentum), float(reg_mf)
        self.adam = E.AdamState(lr)
        self.opt = RowLearner(learner, lr, momentum, self.adam)
        slots = {k: self.opt.slots(getattr(self, k)) for k in _TABLES}
        self.s0, self.s1 = ({k: s[i] for k, s in slots.items()} for i in (0, 1))
        self.flag = {k: self.opt.flag(getattr(self, k).shape[0], dev) for k in _TABLES}
        self.max_batch = int(max_batch)
        N = max(self.max_batch, 1) * (2 if self.pairwise else 1)
        self._keys = torch.empty(3 * N, dtype=torch.int64, device=dev)
        self._scal = torch.empty(4 * max(self.max_batch, 1), dtype=torch.float32, device=dev)
        self.t = 0
        self._factors = None                                   # (step, last_items, P', Q')
        self._scores = ScoreCache()

    def gradients(self, users, recent, items, third, loss_out):
        """the C call alone: loss_out and the batch's rows of self.G (and the row flags); no table moves"""
        B = int(users.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if recent.numel() != B or items.numel() != B or third.numel() != B:
            raise ValueError("users, recent items, items and the fourth field must have the same length")
        a = FpmcStepArgs()
        for k in _TABLES:
            setattr(a, k, _ptr(getattr(self, k)))
            setattr(a, "G_" + k, _ptr(self.G[k]))
            setattr(a, "flag_" + k, addr(self.flag[k]))
        a.users, a.recent, a.items = _ptr(users, torch.int32), _ptr(recent, torch.int32), _ptr(items, torch.int32)
        a.third = _ptr(third, torch.int32 if self.pairwise else torch.float32)
        a.keys, a.scal, a.loss2 = _ptr(self._keys), _ptr(self._scal), _ptr(loss_out, torch.float32)
        a.n_users, a.n_items, a.d, a.batch = self.n_users, self.n_items, self.d, B
        a.pairwise, a.loss_kind, a.reg = int(self.pairwise), self.loss_kind, self.reg_mf
        call("nrhip_fpmc_step", C.byref(a), _stream())

    def apply(self):
        """the four applications of self.G; the gradient rows (and flags) are zero again afterwards"""
        for k in _TABLES:
            self.opt.apply(getattr(self, k), self.s0[k], self.s1[k], self.G[k], self.flag[k])
        self.adam.advance()
        self.t += 1

    def step(self, users, recent, items, third, loss_out):
        """pointwise: third = labels (float32); pairwise: third = negative items (int32).  loss_out: 2 floats on the
        device, (loss term, regulariser term) of the batch before the update."""
        self.gradients(users, recent, items, third, loss_out)
        self.apply()

    # ------------------------------------------------------------------ scoring
    def _last(self, last_items):
        return as_ids(last_items, self.UI.device, self.n_users,
                      "last_items holds {n} entries, the user table {want} rows")

    def user_factors(self, last_items, users=None):
        """[n, 2 d] rows [UI[u] | LI[last_items[u]]] of `users` (int32 device tensor; None: every user); last -1: the
        second half is zeros"""
        n = self.n_users if users is None else int(users.numel())
        out = torch.empty((n, 2 * self.d), dtype=torch.float32, device=self.UI.device)
        call("nrhip_fpmc_user_factors", _ptr(self.UI), _ptr(self.LI), self.n_users, self.n_items, self.d,
             _ptr(last_items, torch.int32), _ptr(users, torch.int32, allow_none=True), n, _ptr(out), out.stride(0),
             _stream())
        return out

    def item_factors(self):
        """[I, 2 d] rows [IU[i] | IL[i]]"""
        out = torch.empty((self.n_items, 2 * self.d), dtype=torch.float32, device=self.UI.device)
        if self.n_items:
            E.copy2d(self.IU, out[:, :self.d])
            E.copy2d(self.IL, out[:, self.d:])
        return out

    def eval_factors(self, last_items):
        """(P' [U, 2 d], Q' [I, 2 d]) whose inner products are predict()'s rows; rebuilt only after a step (or for
        another `last_items` object)"""
        f = self._factors
        if f is None or f[0] != self.t or f[1] is not last_items:
            last = self._last(last_items)
            self._factors = (self.t, last_items, self.user_factors(last), self.item_factors())
        return self._factors[2], self._factors[3]

    def score(self, users, last_items):
        """S [n, I] float32 on the device: FPMC.py:140-152 for `users`, every item, own items included"""
        P = self.user_factors(self._last(last_items), as_ids(users, self.UI.device))
        return self._scores.score(P, self.item_factors(), self.n_items)
