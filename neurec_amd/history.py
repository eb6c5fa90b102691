"""What the engines of the history models share (neurec_amd/fism.py, neurec_amd/nais.py, neurec_amd/fossil.py;
csrc/history_common.h).

A user is not a table row but a pooling of the `c1` rows of the train history; an instance is (user, item, excluded
item or none, count).  Both engines hold c1 / Q / bias, the train matrix and its transpose, one optimiser state per
table, the instance buffers of a batch, and run one C call per step followed by the same applications: `c1` and the
model's dense variables through the dense Apply* kernels (or c1 by rows, `c1_application="rows"`), `embedding_Q` and
`bias` by rows — the forms TF-1.12 picks for tf.concat reads and embedding_lookup reads (neurec_amd/row_learner.py).
`q_application="dense"` gives `embedding_Q` the dense application: the form of a model whose loss also reads the whole
table (DeepICF's regulariser), whose step then leaves a dense gradient in G["Q"].
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import torch

from . import engine as E
from ._lib import call
from .engine import _ptr, _stream
from .row_learner import RowLearner, addr, check_loss_learner, f32


class HistoryEngine:
    """Tables, optimiser state, gradient and instance buffers in HBM, and step().  A subclass names its model (NAME,
    MAX_D), its argument struct and C call (ARGS, STEP), and fills the struct's own fields in `_fill(a)`."""
    NAME, MAX_D, ARGS, STEP = None, 128, None, None

    def __init__(self, c1, Q, train, lr, regs, alpha, max_batch, loss, pairwise, learner, bias, momentum,
                 c1_application, dense=None, sorted_rows=False, q_application="rows"):
        """dense(d): the model's further variables {name: float32 tensor}, checked against embedding_size d — dense
        variables to TF; sorted_rows: de-duplicate the train rows and sort their columns"""
        loss, learner, self.loss_kind = check_loss_learner(loss, learner, pairwise)
        if c1_application not in ("dense", "rows"):
            raise ValueError("c1_application is 'dense' or 'rows', got %r" % (c1_application,))
        if q_application not in ("dense", "rows"):
            raise ValueError("q_application is 'dense' or 'rows', got %r" % (q_application,))
        c1, Q = f32(c1), f32(Q)
        if c1.dim() != 2 or tuple(c1.shape) != tuple(Q.shape):
            raise ValueError("c1 and embedding_Q must both be [num_items, embedding_size]")
        I, d = c1.shape
        if d < 1 or d > self.MAX_D:
            raise NotImplementedError("%s: embedding_size=%d is not supported (1 to %d)" % (self.NAME, d, self.MAX_D))
        more = dense(d) if dense else {}
        M = sp.csr_matrix(train)
        if M.shape[1] != I:
            raise ValueError("train matrix has %d items, the tables %d" % (M.shape[1], I))
        if sorted_rows:
            M.sum_duplicates()
            M.sort_indices()
        dev = E.require_gpu()
        self.loss, self.pairwise, self.learner = loss, bool(pairwise), learner
        self.n_users, self.n_items, self.d = M.shape[0], I, d
        self.csr = E.DeviceCSR.from_scipy(M)
        self.csc = E.DeviceCSR.from_scipy(M.T)                 # item -> its users, ascending
        self.h_deg = np.diff(np.asarray(M.indptr, dtype=np.int64))
        self.c1, self.Q = c1.contiguous().to(dev), Q.contiguous().to(dev)
        self.bias = (torch.zeros(I) if bias is None else f32(bias)).contiguous().to(dev)
        for k, t in more.items():
            setattr(self, k, t.contiguous().to(dev))
        self._dense_names = tuple(more)
        self._names = ("c1", "Q", "bias") + self._dense_names
        self._shared_names = self._names                       # the tables the shared part of the struct names
        self.G = {k: torch.zeros_like(getattr(self, k)) for k in self._names}
        self.lr, self.momentum, self.alpha = float(lr), float(momentum), float(alpha)
        self.reg_p, self.reg_q = float(regs[0]), float(regs[1])
        self.adam = E.AdamState(lr)
        self.opt = RowLearner(learner, lr, momentum, self.adam)
        self.dense = self.opt.dense                           # the dense variables' learner; None: ApplyAdam
        slots = {k: self.opt.slots(getattr(self, k)) for k in self._names}
        self.s0, self.s1 = ({k: s[i] for k, s in slots.items()} for i in (0, 1))
        self.q_dense = q_application == "dense"
        self.flag_Q, self.flag_bias = None if self.q_dense else self.opt.flag(I, dev), self.opt.flag(I, dev)
        # 'rows': c1 gets the sparse application too, on the rows the batch's histories hold (what TF does when the
        # gradient of c1 reaches its optimizer as IndexedSlices); 'dense' (default): the Apply* kernels on every row
        self.c1_rows = c1_application == "rows"
        self.flag_c1 = self.opt.flag(I, dev) if self.c1_rows else None
        self.max_batch = int(max_batch)
        N = self._N = max(self.max_batch, 1) * (2 if self.pairwise else 1)         # instances of the largest batch
        self._keys = torch.empty(2 * N, dtype=torch.int64, device=dev)
        self._inst = torch.empty(4 * N, dtype=torch.int32, device=dev)
        self._n = torch.empty(N, dtype=torch.float32, device=dev)
        self._p = torch.empty((N, d), dtype=torch.float32, device=dev)
        self._scal = torch.empty(8 * N, dtype=torch.float32, device=dev)
        self._slot = torch.zeros(max(self.n_users, 1), dtype=torch.int64, device=dev)
        self.t = 0

    def _apply_rows(self, key, flag):
        self.opt.apply(getattr(self, key), self.s0[key], self.s1[key], self.G[key], flag)

    def _apply_dense(self, keys):
        self.opt.apply_dense([(getattr(self, k), self.s0[k], self.s1[k], self.G[k]) for k in keys], clear_grad=False)

    def _fill(self, a):
        """the fields of the argument struct beyond the shared ones"""

    def _field(self, t, dtype):
        """the device address of a batch field"""
        return _ptr(t, dtype)

    def _shared(self, A):
        """the part of the argument struct that names the fields shared by the history models (the struct itself,
        unless the model's struct nests it)"""
        return A

    def _apply_more(self):
        """the applications of a model's tables beyond c1 / Q / bias and its dense variables"""

    def gradients(self, users, items, third, loss_out):
        """the C call alone: loss_out and the gradient buffers self.G (and the row flags); no table moves"""
        B = int(users.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if items.numel() != B or third.numel() != B:
            raise ValueError("users, items and the third field must have the same length")
        self.t += 1
        A = self.ARGS()
        a = self._shared(A)
        a.indptr, a.indices = _ptr(self.csr.indptr, torch.int64), _ptr(self.csr.indices, torch.int32)
        a.t_indptr, a.t_users = _ptr(self.csc.indptr, torch.int64), _ptr(self.csc.indices, torch.int32)
        for k in self._shared_names:
            setattr(a, k, _ptr(getattr(self, k)))
            setattr(a, "G_" + k, _ptr(self.G[k]))
        a.flag_Q, a.flag_bias, a.flag_c1 = addr(self.flag_Q), addr(self.flag_bias), addr(self.flag_c1)
        a.users, a.items = self._field(users, torch.int32), self._field(items, torch.int32)
        a.third = self._field(third, torch.int32 if self.pairwise else torch.float32)
        a.keys, a.inst, a.n, a.p, a.scal = (_ptr(t) for t in (self._keys, self._inst, self._n, self._p, self._scal))
        a.slot, a.loss2 = _ptr(self._slot), _ptr(loss_out, torch.float32)
        a.n_users, a.n_items, a.d, a.batch = self.n_users, self.n_items, self.d, B
        a.pairwise, a.loss_kind, a.step = int(self.pairwise), self.loss_kind, self.t
        a.alpha, a.reg_p, a.reg_q = self.alpha, self.reg_p, self.reg_q
        self._fill(A)
        call(self.STEP, C.byref(A), _stream())

    def apply(self):
        """the applications of self.G, in the order TF-1.12 runs them here"""
        dense = (("Q",) if self.q_dense else ()) + self._dense_names
        if self.c1_rows:
            self._apply_rows("c1", self.flag_c1)
            self._apply_dense(dense)
        else:
            self._apply_dense(("c1",) + dense)
        if not self.q_dense:
            self._apply_rows("Q", self.flag_Q)
        self._apply_rows("bias", self.flag_bias)
        self._apply_more()
        self.adam.advance()

    def step(self, users, items, third, loss_out):
        """pointwise: third = labels (float32); pairwise: third = negative items (int32).  loss_out: 2 floats on the
        device, (loss term, regulariser term) of the batch before the update."""
        self.gradients(users, items, third, loss_out)
        self.apply()
