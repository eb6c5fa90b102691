"""APR on the HIP engine: the adversarial graph of model/general_recommender/APR.py:73-118 as one optimiser step
(csrc/apr.hip) — Delta of the batch's rows from the plain gradient of this batch (or from a draw), then the gradient
of `opt_loss` with Delta constant.

    x_t = <P[u], Q[i]> - <P[u], Q[j]>        loss = sum softplus(-x_t)
    Delta[row] = eps * normalise(Gamma[row]),   Gamma = d loss / d row over the row's occurrences in the batch
    opt_loss = loss + reg * (sum(P^2) / 2 + sum(Q^2) / 2) + reg_adv * sum softplus(-x~_t)      (the WHOLE tables)

The optimiser forms are TF-1.12's: a step whose tables are read through lookups only (no regulariser, or reg == 0)
takes the sparse application (`RowLearner.apply`: Adam sweeps every row, the other learners move the flagged rows);
with reg != 0 `l2_loss` reads the tables, the gradient is dense and `RowLearner.apply_dense` takes G, whose rows
outside the batch hold reg * row.
"""
import ctypes as C

import torch

from . import engine as E
from ._lib import AprStepArgs, call
from .engine import _ptr, _stream
from .row_learner import RowLearner, addr, check_loss_learner, f32

MAX_D = 128                   # NRHIP_APR_MAX_D
MAX_BATCH = 1 << 24           # NRHIP_APR_MAX_BATCH
L2_BLOCKS = 256               # NRHIP_APR_L2_BLOCKS
ADV = ("grad", "random")      # APR.py:97, 107


def adversarial_epoch(epoch, adver, adv_epoch, reference_train_loop=False):
    """whether the steps of `epoch` (1-based, APR.py:135) perturb: `adver` truthy and epoch > adv_epoch; never in the
    loop as shipped, which minimises `self.loss` whatever the keys say (APR.py:122, 144)"""
    return (not reference_train_loop) and bool(adver) and int(epoch) > int(adv_epoch)


class APREngine:
    """Tables P [U, d] and Q [I, d], their optimiser state, gradient buffers and the step's work buffers in HBM.

    `step(users, pos, neg, loss_out, adversarial=True, with_reg=True)`: one batch of triplets (int32 device tensors);
    loss_out: 2 floats on the device, (loss, opt_loss - loss) at the incoming tables.  `deltas()`: the last
    adversarial step's distinct rows and their Delta rows.  Pairs with pos == neg are allowed."""

    def __init__(self, P, Q, lr, reg, reg_adv, eps, max_batch, adv="grad", learner="adam", momentum=0.9, seed=2018):
        adv = str(adv).lower()
        if adv not in ADV:
            raise ValueError("APR: adv=%r is not supported (one of %s)" % (adv, ", ".join(ADV)))
        _, learner, _ = check_loss_learner("bpr", learner, True)
        P, Q = f32(P), f32(Q)
        if P.dim() != 2 or Q.dim() != 2 or P.shape[1] != Q.shape[1]:
            raise ValueError("P must be [num_users, embedding_size], Q [num_items, embedding_size]")
        (U, d), I = P.shape, Q.shape[0]
        if d < 1 or d > MAX_D:
            raise NotImplementedError("APR: embedding_size=%d is not supported (1 to %d)" % (d, MAX_D))
        if int(max_batch) > MAX_BATCH:
            raise ValueError("APR: max_batch=%d is not supported (at most %d)" % (max_batch, MAX_BATCH))
        dev = E.require_gpu()
        self.adv, self.learner = adv, learner
        self.n_users, self.n_items, self.d = U, I, d
        self.P, self.Q = P.contiguous().to(dev), Q.contiguous().to(dev)
        self.GP, self.GQ = torch.zeros_like(self.P), torch.zeros_like(self.Q)
        self.lr, self.reg, self.reg_adv, self.eps = float(lr), float(reg), float(reg_adv), float(eps)
        self.adam = E.AdamState(lr)
        self.opt = RowLearner(learner, lr, momentum, self.adam)
        (self.s0P, self.s1P), (self.s0Q, self.s1Q) = self.opt.slots(self.P), self.opt.slots(self.Q)
        self.flagP, self.flagQ = self.opt.flag(U, dev), self.opt.flag(I, dev)
        self.max_batch = int(max_batch)
        n = 3 * max(self.max_batch, 1)
        self._keys = torch.empty(n, dtype=torch.int64, device=dev)
        self._scal = torch.empty(4 * max(self.max_batch, 1), dtype=torch.float32, device=dev)
        self._where = torch.empty(n, dtype=torch.int32, device=dev)
        self._gamma = torch.empty((n, d), dtype=torch.float32, device=dev)
        self._delta = torch.empty((n, d), dtype=torch.float32, device=dev)
        self._part = torch.empty(L2_BLOCKS, dtype=torch.float64, device=dev)
        self.seed = int(seed)
        self.t = 0
        self._dense = False                                    # the form of the gradient that lies in GP / GQ
        self._last = None                                      # (batch, adversarial) of the last gradients()

    def gradients(self, users, pos, neg, loss_out, adversarial=True, with_reg=True, delta_given=None):
        """the C call alone: loss_out, self.GP / self.GQ (and the row flags); no table moves.  delta_given: (rows_P,
        Delta_P, rows_Q, Delta_Q) as `deltas()` returns them, in place of the step's own Delta"""
        B = int(users.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if pos.numel() != B or neg.numel() != B:
            raise ValueError("users, positive items and negative items must have the same length")
        dense = bool(with_reg) and self.reg != 0.0
        given = None
        if delta_given is not None and adversarial:
            rows_p, dp, rows_q, dq = delta_given
            given = torch.zeros((self.n_users + self.n_items, self.d), dtype=torch.float32, device=self.P.device)
            given[rows_p.long()] = dp.to(given)
            given[rows_q.long() + self.n_users] = dq.to(given)
        a = AprStepArgs()
        a.P, a.Q, a.G_P, a.G_Q = _ptr(self.P), _ptr(self.Q), _ptr(self.GP), _ptr(self.GQ)
        a.flag_P, a.flag_Q = (None, None) if dense else (addr(self.flagP), addr(self.flagQ))
        a.users, a.pos, a.neg = _ptr(users, torch.int32), _ptr(pos, torch.int32), _ptr(neg, torch.int32)
        a.delta_given = addr(given)
        a.keys, a.scal, a.where = _ptr(self._keys), _ptr(self._scal), _ptr(self._where)
        a.gamma, a.delta, a.part = _ptr(self._gamma), _ptr(self._delta), _ptr(self._part)
        a.loss2 = _ptr(loss_out, torch.float32)
        a.seed, a.step = self.seed, self.t
        a.n_users, a.n_items, a.d, a.batch = self.n_users, self.n_items, self.d, B
        a.adversarial, a.adv_random, a.with_reg = int(bool(adversarial)), int(self.adv == "random"), int(bool(with_reg))
        a.reg, a.reg_adv, a.eps = self.reg, self.reg_adv, self.eps
        if B == 0 and not dense:
            loss_out.zero_()                                   # the call launches nothing for an empty batch
        call("nrhip_apr_step", C.byref(a), _stream())
        self._dense, self._last = dense, (B, bool(adversarial))

    def apply(self):
        """the two applications of self.GP / self.GQ in the form the last gradients() left; the gradients (and the
        flags) are zero again afterwards"""
        tabs = ((self.P, self.s0P, self.s1P, self.GP, self.flagP), (self.Q, self.s0Q, self.s1Q, self.GQ, self.flagQ))
        if self._dense:
            self.opt.apply_dense([t[:4] for t in tabs], True)
        else:
            for var, s0, s1, grad, flag in tabs:
                self.opt.apply(var, s0, s1, grad, flag)
        self.adam.advance()
        self.t += 1

    def step(self, users, pos, neg, loss_out, adversarial=True, with_reg=True, delta_given=None):
        self.gradients(users, pos, neg, loss_out, adversarial, with_reg, delta_given)
        self.apply()

    def deltas(self):
        """(rows_P, Delta_P, rows_Q, Delta_Q) of the last adversarial gradients(): the batch's distinct rows of each
        table, ascending, and their perturbations.  For tests: it reads the sorted keys back"""
        if self._last is None or not self._last[1]:
            raise ValueError("APR: the last step was not adversarial")
        n = 3 * self._last[0]
        keys = self._keys[:n]
        rows = keys >> 32
        head = keys != 0x7fffffffffffffff
        if n > 1:
            head[1:] &= rows[1:] != rows[:-1]
        at = torch.nonzero(head).reshape(-1)
        rows, delta = rows[at], self._delta[at]
        user = rows < self.n_users
        return (rows[user].to(torch.int32), delta[user].clone(),
                (rows[~user] - self.n_users).to(torch.int32), delta[~user].clone())

    def tables(self):
        return self.P, self.Q
