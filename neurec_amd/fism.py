"""FISM on the HIP engine: the graph of FISM.py:55-92 and one `sess.run((loss, optimizer))` per step (csrc/fism.hip).

A user is not a table row but the sum of the `c1` rows of the train history, minus the target item for a positive
instance.  The reference pads every batch to [B, Lmax] and gathers [B, Lmax, d]; here a wave walks the user's CSR row
(forward) and a wave per item walks the transposed train matrix against the batch's users (backward), so neither the
padded id matrix nor the gathered block exist.

Optimiser forms, as TF-1.12 picks them: `c1` is read through tf.concat, so its gradient is dense and the dense Apply*
kernels run on every row each step (ApplyAdam; the other learners decay or move untouched rows too); `embedding_Q` and
`bias` are read through embedding_lookup and get the sparse application GeneralMFEngine uses for MF.  That is what the
TensorFlow stand-in's trace records; `c1_application="rows"` gives c1 the sparse application as well.
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from ._lib import FismStepArgs, call
from .engine import _ptr, _stream
from .history import HistoryEngine

MAX_D = 128                   # NRHIP_FISM_MAX_D


class FISMEngine(HistoryEngine):
    """Tables c1 / Q / bias, their optimiser state and gradient buffers in HBM (neurec_amd/history.py).

    `step(users, items, third, loss_out)`: one batch of the device instance stream — pointwise (third = float labels;
    label 1: history without the item, n = |R_u|; label 0: whole history, n = |R_u| + 1) or pairwise (third = int32
    negatives; users with a single train item take no part).  `score(users)` -> [B, I] on the device."""
    NAME, MAX_D, ARGS, STEP = "FISM", MAX_D, FismStepArgs, "nrhip_fism_step"

    def __init__(self, c1, Q, train, lr, regs, alpha, max_batch, loss="square", pairwise=False, learner="adam",
                 bias=None, momentum=0.9, c1_application="dense"):
        HistoryEngine.__init__(self, c1, Q, train, lr, regs, alpha, max_batch, loss, pairwise, learner, bias, momentum,
                               c1_application)
        self._g = torch.empty((self._N, self.d), dtype=torch.float32, device=self.c1.device)
        self._factors = None                                   # (step they were made at, users, items)
        self._items = None                                     # (step, [Q | bias]) of score()
        self._gemm = None

    def _fill(self, a):
        a.g = _ptr(self._g)

    # ------------------------------------------------------------------ scoring
    def user_factors(self, users=None):
        """[B, d + 1] rows [|R_u|^-alpha p_u | 1] of `users` (int32 device tensor; None: every user)"""
        B = self.n_users if users is None else int(users.numel())
        out = torch.empty((B, self.d + 1), dtype=torch.float32, device=self.c1.device)
        call("nrhip_fism_user_factors", _ptr(self.csr.indptr), _ptr(self.csr.indices), self.n_users, _ptr(self.c1),
             self.d, C.c_float(self.alpha), _ptr(users, torch.int32, allow_none=True), B, _ptr(out), out.stride(0),
             _stream())
        return out

    def item_factors(self):
        """[I, d + 1] rows [Q[i] | bias[i]]"""
        return torch.cat([self.Q, self.bias.reshape(-1, 1)], dim=1).contiguous()

    def eval_factors(self):
        """(user factors [U, d + 1], item factors [I, d + 1]) whose inner products are predict()'s rows; made once per
        table state"""
        if self._factors is None or self._factors[0] != self.t:
            if self._items is None or self._items[0] != self.t:
                self._items = (self.t, self.item_factors())
            self._factors = (self.t, self.user_factors(), self._items[1])
        return self._factors[1], self._factors[2]

    def score(self, users):
        """S [B, I] float32 on the device: FISM.py:168-179 for `users`, every item, own items included"""
        dev = self.c1.device
        if not isinstance(users, torch.Tensor):
            users = torch.from_numpy(np.ascontiguousarray(users, dtype=np.int32))
        users = users.to(dev, torch.int32).contiguous()
        B = int(users.numel())
        if self._items is None or self._items[0] != self.t:
            self._items = (self.t, self.item_factors())
        items = self._items[1]
        if self._gemm is None or self._gemm[0].max_rows < B:
            self._gemm = [E.score_gemm_for(items, max(B, 1)), self.t]
        elif self._gemm[1] != self.t:
            self._gemm[0].prepare(items)
            self._gemm[1] = self.t
        return self._gemm[0](self.user_factors(users), None)[:, :self.n_items]
