"""FPMCplus on the HIP engine: the graph of model/sequential_recommender/FPMCplus.py:73-119 and one
`sess.run((loss, optimizer))` per step, and predict() (csrc/fpmcplus.hip).

An instance is (user, recents r_0..r_{L-1}, item[, negative]).  FPMC's four tables plus an attention MLP (W [3d, w],
b [1, w], h [w, 1]) that weights the L recents per target item:
    a_l = tanh([UI_u | IL_i | LI_{r_l}] W + b),  alpha = softmax_l(a_l h),  x(u, i) = <UI_u, IU_i> + <IL_i, sum_l alpha_l LI_{r_l}>
The attention depends on the target item, so the score has no factor form: evaluation has a kernel of its own, as NAIS.

Optimiser forms, as TF-1.12 picks them: the four tables are read through embedding_lookup only — the sparse
application (neurec_amd/row_learner.py); W, b and h are read through matmul — the dense Apply* kernels, every step.
"""
import ctypes as C

import torch

from . import engine as E
from ._lib import FpmcplusScoresArgs, FpmcplusStepArgs, call
from .engine import _ptr, _stream
from .model._common import last_items_table            # noqa: F401  (predict()'s table, made by the plugin)
from .row_learner import RowLearner, addr, as_ids, check_loss_learner, f32

MAX_D = 128                   # NRHIP_FPMCPLUS_MAX_D
MAX_W = 64                    # NRHIP_FPMCPLUS_MAX_W
MAX_L = 16                    # NRHIP_FPMCPLUS_MAX_L
MAX_CHUNKS = 64               # NRHIP_FPMCPLUS_MAX_CHUNKS
_ROWS = ("UI", "IU", "IL", "LI")
_DENSE = ("W", "b", "h")
_TABLES = _ROWS + _DENSE


class FPMCplusEngine:
    """Tables UI [U, d], IU / IL / LI [I, d], W [3d, w], b [w], h [w], their optimiser state and gradient buffers in HBM.

    `step(users, recents [B, L], items, third, loss_out)`: one batch of the time-order instance stream at
    high_order = L — pointwise (third = float labels) or pairwise (third = int32 negatives).  `score(users)` -> [n, I]
    on the device, from the [U, L] last-items table."""

    def __init__(self, UI, IU, IL, LI, W, b, h, lr, reg_mf, reg_w, max_batch, high_order, loss="bpr", pairwise=True,
                 learner="adam", momentum=0.9, last_items=None):
        loss, learner, self.loss_kind = check_loss_learner(loss, learner, pairwise)
        UI, IU, IL, LI, W = f32(UI), f32(IU), f32(IL), f32(LI), f32(W)
        if UI.dim() != 2 or IU.dim() != 2 or IU.shape[1] != UI.shape[1] or \
                tuple(IL.shape) != tuple(IU.shape) or tuple(LI.shape) != tuple(IU.shape):
            raise ValueError("UI must be [num_users, embedding_size], IU / IL / LI [num_items, embedding_size]")
        (U, d), I = UI.shape, IU.shape[0]
        if d < 1 or d > MAX_D:
            raise NotImplementedError("FPMCplus: embedding_size=%d is not supported (1 to %d)" % (d, MAX_D))
        if W.dim() != 2 or W.shape[0] != 3 * d:
            raise ValueError("W must be [3 * embedding_size, weight_size] = [%d, weight_size]" % (3 * d,))
        w = int(W.shape[1])
        if w < 1 or w > MAX_W:
            raise NotImplementedError("FPMCplus: weight_size=%d is not supported (1 to %d)" % (w, MAX_W))
        b, h = f32(b).reshape(-1), f32(h).reshape(-1)
        if b.numel() != w or h.numel() != w:
            raise ValueError("b and h must hold weight_size entries")
        L = int(high_order)
        if L < 1 or L > MAX_L:
            raise NotImplementedError("FPMCplus: high_order=%d is not supported (1 to %d)" % (L, MAX_L))
        dev = E.require_gpu()
        self.loss, self.pairwise, self.learner = loss, bool(pairwise), learner
        self.n_users, self.n_items, self.d, self.w, self.L = U, I, d, w, L
        self.UI, self.IU, self.IL, self.LI, self.W, self.b, self.h = \
            (t.contiguous().to(dev) for t in (UI, IU, IL, LI, W, b, h))
        self.G = {k: torch.zeros_like(getattr(self, k)) for k in _TABLES}
        self.lr, self.momentum = float(lr), float(momentum)
        self.reg_mf, self.reg_w = float(reg_mf), float(reg_w)
        self.adam = E.AdamState(lr)
        self.opt = RowLearner(learner, lr, momentum, self.adam)
        self.dense = self.opt.dense                           # W, b, h; None: ApplyAdam
        slots = {k: self.opt.slots(getattr(self, k)) for k in _TABLES}
        self.s0, self.s1 = ({k: s[i] for k, s in slots.items()} for i in (0, 1))
        self.flag = {k: self.opt.flag(getattr(self, k).shape[0], dev) for k in _ROWS}
        self.max_batch = int(max_batch)
        mb = max(self.max_batch, 1)
        K = (5 if self.pairwise else 3) + L                    # looked-up rows per instance
        self._keys = torch.empty(K * mb, dtype=torch.int64, device=dev)
        self._contrib = torch.empty((K * mb, d), dtype=torch.float32, device=dev)
        self._scal = torch.empty(4 * mb, dtype=torch.float32, device=dev)
        self._delta = torch.empty((mb, (L + 4) * w), dtype=torch.float32, device=dev)
        self._partial = torch.empty((min((mb + 31) // 32, MAX_CHUNKS), 3 * d * w + 2 * w), dtype=torch.float32,
                                    device=dev)
        self.t = 0
        self.last_items = None
        self._c = self._p = None                               # score()'s workspace
        if last_items is not None:
            self.set_last_items(last_items)

    def set_last_items(self, last_items):
        """the [U, L] table of predict(): the user's last min(|R_u|, L) items, -1 where there is none"""
        last_items = as_ids(last_items, self.UI.device)
        if tuple(last_items.shape) != (self.n_users, self.L):
            raise ValueError("last items must be [num_users, high_order] = [%d, %d], got %s"
                             % (self.n_users, self.L, tuple(last_items.shape)))
        self.last_items = last_items

    # ------------------------------------------------------------------ training
    def gradients(self, users, recents, items, third, loss_out):
        """the C call alone: loss_out, the batch's rows of self.G (and the row flags) and G_W / G_b / G_h whole; no
        table moves.  An empty batch is no work: nothing is launched and loss_out is set to zero."""
        B = int(users.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if items.numel() != B or third.numel() != B:
            raise ValueError("users, items and the fourth field must have the same length")
        if recents.numel() != B * self.L or (recents.dim() == 2 and tuple(recents.shape) != (B, self.L)):
            raise ValueError("recents must be [batch, high_order] = [%d, %d], got %s"
                             % (B, self.L, tuple(recents.shape)))
        if B == 0:
            loss_out.zero_()
            return
        a = FpmcplusStepArgs()
        for k in _TABLES:
            setattr(a, k, _ptr(getattr(self, k)))
            setattr(a, "G_" + k, _ptr(self.G[k]))
        for k in _ROWS:
            setattr(a, "flag_" + k, addr(self.flag[k]))
        a.users, a.recents, a.items = _ptr(users, torch.int32), _ptr(recents, torch.int32), _ptr(items, torch.int32)
        a.third = _ptr(third, torch.int32 if self.pairwise else torch.float32)
        a.keys, a.contrib, a.scal = _ptr(self._keys), _ptr(self._contrib), _ptr(self._scal)
        a.delta, a.partial, a.loss2 = _ptr(self._delta), _ptr(self._partial), _ptr(loss_out, torch.float32)
        a.n_users, a.n_items, a.d, a.w, a.L, a.batch = self.n_users, self.n_items, self.d, self.w, self.L, B
        a.pairwise, a.loss_kind, a.reg_mf, a.reg_w = int(self.pairwise), self.loss_kind, self.reg_mf, self.reg_w
        call("nrhip_fpmcplus_step", C.byref(a), _stream())

    def apply(self):
        """the seven applications of self.G; the gradient buffers (and flags) are zero again afterwards"""
        for k in _ROWS:
            self.opt.apply(getattr(self, k), self.s0[k], self.s1[k], self.G[k], self.flag[k])
        self.opt.apply_dense([(getattr(self, k), self.s0[k], self.s1[k], self.G[k]) for k in _DENSE], clear_grad=True)
        self.adam.advance()
        self.t += 1

    def step(self, users, recents, items, third, loss_out):
        """pointwise: third = labels (float32); pairwise: third = negative items (int32).  loss_out: 2 floats on the
        device, (loss term, regulariser term) of the batch before the update.  An empty batch moves nothing, the
        step counter included."""
        self.gradients(users, recents, items, third, loss_out)
        if int(users.numel()):
            self.apply()

    # ------------------------------------------------------------------ scoring
    def score(self, users):
        """S [n, I] float32 on the device: FPMCplus.py:177-191 for `users`, every item, own items included"""
        if self.last_items is None:
            raise ValueError("score() needs the last items table: pass last_items= or call set_last_items()")
        dev = self.UI.device
        users = as_ids(users, dev)
        n, I = int(users.numel()), self.n_items
        out = torch.empty((n, I), dtype=torch.float32, device=dev)
        if n == 0 or I == 0:
            return out
        if self._p is None:
            self._p = torch.empty((I, self.w), dtype=torch.float32, device=dev)
        if self._c is None or self._c.shape[0] < n:
            self._c = None
            self._c = torch.empty((n, self.L * self.w), dtype=torch.float32, device=dev)
        a = FpmcplusScoresArgs()
        for k in _TABLES:
            setattr(a, k, _ptr(getattr(self, k)))
        a.last, a.users = _ptr(self.last_items, torch.int32), _ptr(users, torch.int32)
        a.c, a.p, a.out, a.ld = _ptr(self._c), _ptr(self._p), _ptr(out), out.stride(0)
        a.n_users, a.n_items, a.d, a.w, a.L, a.batch = self.n_users, I, self.d, self.w, self.L, n
        call("nrhip_fpmcplus_scores", C.byref(a), _stream())
        return out
