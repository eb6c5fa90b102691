"""Fossil on the HIP engine: the graph of model/sequential_recommender/Fossil.py:59-102 and one
`sess.run((loss, optimizer))` per step (csrc/fossil.hip).

An instance is (user, item, excluded item or none, count, L recents): FISM's pooled history (neurec_amd/history.py)
plus a personalised Markov term, s = sum_l (eta_bias[l] + eta[u, l]) c1[r_l], over the same c1 table,
    out = n^-alpha <p, Q[i]> + <s, Q[i]> + bias[i].
The recents come MOST RECENT FIRST: column l of `recents` meets column l of eta.

Optimiser forms, as TF-1.12 picks them: `c1` is read through tf.concat (by both routes, the history and the recents),
so its gradient is dense and the dense Apply* kernels run on every row; `eta_bias` is a dense variable; `embedding_Q`,
`bias` and the per-user table `eta` are read through embedding_lookup and get the sparse application.

The score has a factor form, [ |R_u|^-alpha p_u + s_u | 1 ] . [Q[i] | bias[i]]: evaluation is the factor path at width
d + 1 with s_u over a [U, L] table of the users' last items.
"""
import ctypes as C

import torch

from ._lib import FossilStepArgs, call
from .engine import _ptr, _stream
from .history import HistoryEngine
from .row_learner import ScoreCache, addr, as_ids, f32

MAX_D = 128                   # NRHIP_FOSSIL_MAX_D
MAX_ORDER = 16                # NRHIP_FOSSIL_MAX_ORDER


class FossilEngine(HistoryEngine):
    """Tables c1 / Q / bias / eta [U, L] / eta_bias [L], their optimiser state and gradient buffers in HBM.

    `step(users, recents, items, third, loss_out)`: one batch of the time-order instance stream at high_order = L,
    recents [B, L] most recent first — pointwise (third = float labels; label 1: history without the item,
    n = |R_u| - 1; label 0: whole history, n = |R_u|) or pairwise (third = int32 negatives).  Users with |R_u| <= L and
    slots with a recent outside the user's train row take no part.  `score(users)` -> [B, I] on the device."""
    NAME, MAX_D, ARGS, STEP = "Fossil", MAX_D, FossilStepArgs, "nrhip_fossil_step"

    def __init__(self, c1, Q, eta, eta_bias, train, lr, regs, alpha, max_batch, loss="bpr", pairwise=True,
                 learner="adagrad", bias=None, momentum=0.9, last_items=None):
        eta = f32(eta)
        if eta.dim() != 2:
            raise ValueError("eta must be [num_users, high_order]")
        U, L = eta.shape
        if L < 1 or L > MAX_ORDER:
            raise NotImplementedError("Fossil: high_order=%d is not supported (1 to %d)" % (L, MAX_ORDER))
        if len(regs) < 3:
            raise ValueError("regs holds three entries: the pooled history's, the embeddings' and eta's")

        def dense(d):
            eb = f32(eta_bias).reshape(-1)
            if eb.numel() != L:
                raise ValueError("eta_bias must hold high_order entries")
            return {"eta_bias": eb}
        # sorted rows: the step finds a recent in its user's row by bisection
        HistoryEngine.__init__(self, c1, Q, train, lr, regs, alpha, max_batch, loss, pairwise, learner, bias, momentum,
                               "dense", dense=dense, sorted_rows=True)
        if U != self.n_users:
            raise ValueError("eta has %d rows, the train matrix %d users" % (U, self.n_users))
        dev, d, N = self.c1.device, self.d, self._N
        self.L, self.reg_eta = L, float(regs[2])
        self.eta = eta.contiguous().to(dev)
        self.G["eta"] = torch.zeros_like(self.eta)
        self.s0["eta"], self.s1["eta"] = self.opt.slots(self.eta)
        self.flag_eta = self.opt.flag(max(U, 1), dev)
        self._g = torch.empty((N, d), dtype=torch.float32, device=dev)
        self._x = torch.empty((N, d), dtype=torch.float32, device=dev)
        self._dots = torch.empty((N, L), dtype=torch.float32, device=dev)
        self._recents = None
        self._nothing = {t: torch.zeros(L, dtype=t, device=dev) for t in (torch.int32, torch.float32)}
        self.last_items = None if last_items is None else self._last(last_items)   # score()'s default
        self._factors = None                                   # (step, last_items, users' factors, items' factors)
        self._scores = ScoreCache()

    def _field(self, t, dtype):
        # an empty batch is a step too (eta_bias's regulariser enters once per step): the C call wants an address
        return _ptr(t if t.numel() else self._nothing[dtype], dtype)

    def _fill(self, a):
        a.eta, a.G_eta, a.flag_eta = _ptr(self.eta), _ptr(self.G["eta"]), addr(self.flag_eta)
        a.recents = self._field(self._recents, torch.int32)
        a.g, a.x, a.dots = _ptr(self._g), _ptr(self._x), _ptr(self._dots)
        a.L, a.reg_eta = self.L, self.reg_eta

    def _apply_more(self):
        self.opt.apply(self.eta, self.s0["eta"], self.s1["eta"], self.G["eta"], self.flag_eta)

    def gradients(self, users, recents, items, third, loss_out):
        """the C call alone: loss_out and the gradient buffers self.G (and the row flags); no table moves"""
        B = int(users.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if recents.numel() != B * self.L:
            raise ValueError("recents must hold high_order = %d entries per slot" % self.L)
        self._recents = recents
        try:
            HistoryEngine.gradients(self, users, items, third, loss_out)
        finally:
            self._recents = None

    def step(self, users, recents, items, third, loss_out):
        """recents: int32 [B, L] (or [B] when L = 1), most recent first.  pointwise: third = labels (float32);
        pairwise: third = negative items (int32).  loss_out: 2 floats on the device, (loss term, regulariser term) of
        the batch before the update."""
        self.gradients(users, recents, items, third, loss_out)
        self.apply()

    # ------------------------------------------------------------------ scoring
    def _last(self, last_items):
        return as_ids(last_items, self.c1.device, self.n_users * self.L,
                      "last_items holds {n} entries, not [num_users, high_order] = [%d, %d]" % (self.n_users, self.L))

    def user_factors(self, last_items, users=None):
        """[B, d + 1] rows [ |R_u|^-alpha p_u + sum_l w_{u,l} c1[last_items[u, l]] | 1 ] of `users` (int32 device
        tensor; None: every user); last_items: int32 [U, L] on the device, -1: the zero row"""
        B = self.n_users if users is None else int(users.numel())
        out = torch.empty((B, self.d + 1), dtype=torch.float32, device=self.c1.device)
        call("nrhip_fossil_user_factors", _ptr(self.csr.indptr), _ptr(self.csr.indices), self.n_users, self.n_items,
             _ptr(self.c1), _ptr(self.eta), _ptr(self.eta_bias), _ptr(last_items, torch.int32), self.d, self.L,
             C.c_float(self.alpha), _ptr(users, torch.int32, allow_none=True), B, _ptr(out), out.stride(0), _stream())
        return out

    def item_factors(self):
        """[I, d + 1] rows [Q[i] | bias[i]]"""
        return torch.cat([self.Q, self.bias.reshape(-1, 1)], dim=1).contiguous()

    def eval_factors(self, last_items):
        """(user factors [U, d + 1], item factors [I, d + 1]) whose inner products are predict()'s rows; rebuilt only
        after a step (or for another `last_items` object)"""
        f = self._factors
        if f is None or f[0] != self.t or f[1] is not last_items:
            self._factors = (self.t, last_items, self.user_factors(self._last(last_items)), self.item_factors())
        return self._factors[2], self._factors[3]

    def score(self, users, last_items=None):
        """S [B, I] float32 on the device: Fossil.py:177-217 for `users`, every item, own items included; last_items
        None: the table the engine was built with"""
        if last_items is None:
            if self.last_items is None:
                raise ValueError("score() needs the [num_users, high_order] table of last items")
            last_items = self.last_items
        P = self.user_factors(self._last(last_items), as_ids(users, self.c1.device))
        return self._scores.score(P, self.item_factors(), self.n_items)
