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
import scipy.sparse as sp
import torch

from . import engine as E
from ._lib import FismStepArgs, call
from .engine import _ptr, _stream

MAX_D = 128                   # NRHIP_FISM_MAX_D


def _addr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class FISMEngine:
    """Tables c1 / Q / bias, their optimiser state and gradient buffers in HBM.

    `step(users, items, third, loss_out)`: one batch of the device instance stream — pointwise (third = float labels;
    label 1: history without the item, n = |R_u|; label 0: whole history, n = |R_u| + 1) or pairwise (third = int32
    negatives; users with a single train item take no part).  `score(users)` -> [B, I] on the device."""

    def __init__(self, c1, Q, train, lr, regs, alpha, max_batch, loss="square", pairwise=False, learner="adam",
                 bias=None, momentum=0.9, c1_application="dense"):
        loss, learner = str(loss).lower(), str(learner).lower()
        table = E.PAIRWISE_LOSSES if pairwise else E.POINTWISE_LOSSES
        if loss not in table:
            raise Exception("please choose a suitable loss function")        # learner.py:28,40
        if learner != "adam" and learner not in E.ROW_OPTIMIZERS:
            raise ValueError("please select a suitable optimizer")           # learner.py:15
        if c1_application not in ("dense", "rows"):
            raise ValueError("c1_application is 'dense' or 'rows', got %r" % (c1_application,))
        c1 = torch.as_tensor(np.asarray(c1), dtype=torch.float32)
        Q = torch.as_tensor(np.asarray(Q), dtype=torch.float32)
        if c1.dim() != 2 or tuple(c1.shape) != tuple(Q.shape):
            raise ValueError("c1 and embedding_Q must both be [num_items, embedding_size]")
        I, d = c1.shape
        if d < 1 or d > MAX_D:
            raise NotImplementedError("FISM: embedding_size=%d is not supported (1 to %d)" % (d, MAX_D))
        M = sp.csr_matrix(train)
        if M.shape[1] != I:
            raise ValueError("train matrix has %d items, the tables %d" % (M.shape[1], I))
        dev = E.require_gpu()
        self.loss, self.pairwise, self.learner = loss, bool(pairwise), learner
        self.loss_kind = table[loss]
        self.n_users, self.n_items, self.d = M.shape[0], I, d
        self.csr = E.DeviceCSR.from_scipy(M)
        self.csc = E.DeviceCSR.from_scipy(M.T)                 # item -> its users, ascending
        self.c1, self.Q = c1.contiguous().to(dev), Q.contiguous().to(dev)
        self.bias = (torch.zeros(I) if bias is None else torch.as_tensor(np.asarray(bias), dtype=torch.float32)) \
            .contiguous().to(dev)
        self.G_c1, self.G_Q, self.G_bias = (torch.zeros_like(t) for t in (self.c1, self.Q, self.bias))
        self.lr, self.momentum, self.alpha = float(lr), float(momentum), float(alpha)
        self.reg_p, self.reg_q = float(regs[0]), float(regs[1])
        self.adam = E.AdamState(lr)
        self.dense = E.make_learner(learner, lr)               # c1's learner; None: ApplyAdam
        init = {"adam": 0.0, "gd": None, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        two = learner in ("adam", "rmsprop")
        mk = lambda t, v: None if v is None else torch.full_like(t, v)
        self.s0 = {k: mk(t, init) for k, t in (("c1", self.c1), ("Q", self.Q), ("bias", self.bias))}
        self.s1 = {k: (mk(t, 0.0) if two else None) for k, t in (("c1", self.c1), ("Q", self.Q), ("bias", self.bias))}
        rows = learner != "adam"
        self.flag_Q = torch.zeros(I, dtype=torch.uint8, device=dev) if rows else None
        self.flag_bias = torch.zeros(I, dtype=torch.uint8, device=dev) if rows else None
        # 'rows': c1 gets the sparse application too, on the rows the batch's histories hold (what TF does when the
        # gradient of c1 reaches its optimizer as IndexedSlices); 'dense' (default): the Apply* kernels on every row
        self.c1_rows = c1_application == "rows"
        self.flag_c1 = torch.zeros(I, dtype=torch.uint8, device=dev) if (rows and self.c1_rows) else None
        self.max_batch = int(max_batch)
        N = max(self.max_batch, 1) * (2 if self.pairwise else 1)
        self._keys = torch.empty(2 * N, dtype=torch.int64, device=dev)
        self._inst = torch.empty(4 * N, dtype=torch.int32, device=dev)
        self._n = torch.empty(N, dtype=torch.float32, device=dev)
        self._p = torch.empty((N, d), dtype=torch.float32, device=dev)
        self._g = torch.empty((N, d), dtype=torch.float32, device=dev)
        self._scal = torch.empty(8 * N, dtype=torch.float32, device=dev)
        self._slot = torch.zeros(max(self.n_users, 1), dtype=torch.int64, device=dev)
        self.t = 0
        self._factors = None                                   # (step they were made at, users, items)
        self._items = None                                     # (step, [Q | bias]) of score()
        self._gemm = None

    # ------------------------------------------------------------------ training
    def _apply_rows(self, var, key, grad, flag):
        s0, s1 = self.s0[key], self.s1[key]
        var2, grad2 = var.view(self.n_items, -1), grad.view(self.n_items, -1)
        v2 = lambda s: None if s is None else s.view(self.n_items, -1)
        if self.learner == "adam":
            E.adam_sparse(var, s0, s1, grad, self.adam)
        elif self.learner == "rmsprop":
            E.optimizer_rows("rmsprop", var2, v2(s0), v2(s1), grad2, flag, self.lr, 0.9, 0.0, 1e-10)
        elif self.learner == "momentum":
            E.optimizer_rows("momentum", var2, v2(s0), None, grad2, flag, self.lr, self.momentum)
        else:
            E.optimizer_rows(self.learner, var2, v2(s0), None, grad2, flag, self.lr)

    def step(self, users, items, third, loss_out):
        """pointwise: third = labels (float32); pairwise: third = negative items (int32).  loss_out: 2 floats on the
        device, (loss term, regulariser term) of the batch before the update."""
        B = int(users.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if items.numel() != B or third.numel() != B:
            raise ValueError("users, items and the third field must have the same length")
        self.t += 1
        a = FismStepArgs()
        a.indptr, a.indices = _ptr(self.csr.indptr, torch.int64), _ptr(self.csr.indices, torch.int32)
        a.t_indptr, a.t_users = _ptr(self.csc.indptr, torch.int64), _ptr(self.csc.indices, torch.int32)
        a.c1, a.Q, a.bias = _ptr(self.c1), _ptr(self.Q), _ptr(self.bias)
        a.G_c1, a.G_Q, a.G_bias = _ptr(self.G_c1), _ptr(self.G_Q), _ptr(self.G_bias)
        a.flag_Q, a.flag_bias, a.flag_c1 = _addr(self.flag_Q), _addr(self.flag_bias), _addr(self.flag_c1)
        a.users, a.items = _ptr(users, torch.int32), _ptr(items, torch.int32)
        a.third = _ptr(third, torch.int32 if self.pairwise else torch.float32)
        a.keys, a.inst, a.n, a.p, a.g = _ptr(self._keys), _ptr(self._inst), _ptr(self._n), _ptr(self._p), _ptr(self._g)
        a.scal, a.slot, a.loss2 = _ptr(self._scal), _ptr(self._slot), _ptr(loss_out, torch.float32)
        a.n_users, a.n_items, a.d, a.batch = self.n_users, self.n_items, self.d, B
        a.pairwise, a.loss_kind, a.step = int(self.pairwise), self.loss_kind, self.t
        a.alpha, a.reg_p, a.reg_q = self.alpha, self.reg_p, self.reg_q
        call("nrhip_fism_step", C.byref(a), _stream())
        if self.c1_rows:
            self._apply_rows(self.c1, "c1", self.G_c1, self.flag_c1)
        elif self.dense is None:
            E.adam_dense(self.c1, self.s0["c1"], self.s1["c1"], self.G_c1, self.adam, clear_grad=False)
        else:
            self.dense.apply([(self.c1, self.s0["c1"], self.s1["c1"], self.G_c1, False)])
        self._apply_rows(self.Q, "Q", self.G_Q, self.flag_Q)
        self._apply_rows(self.bias, "bias", self.G_bias, self.flag_bias)
        self.adam.advance()

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
