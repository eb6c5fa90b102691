"""util/learner.py as TF-1.12 runs it on a variable that is read through embedding_lookup only — stated once for every
engine whose tables are such variables (GeneralMFEngine, HistoryEngine and its models, FPMC, HRM, NPE, TransRec,
FPMCplus) — and the small host helpers those engines share.

The gradient of such a variable is IndexedSlices, so the optimiser takes its sparse form: Adam sweeps every row
(`E.adam_sparse`), gd / adagrad / rmsprop / momentum move only the rows the batch touched (`E.optimizer_rows`, by row
flags that the step kernels set).  A variable read through a dense op (tf.concat, tf.tile, matmul) gets the dense
Apply* kernels instead: `RowLearner.apply_dense`.
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E


def check_loss_learner(loss, learner, pairwise):
    """(loss, learner) lower-cased and `loss`'s code in the C calls; the refusals of learner.py"""
    loss, learner = str(loss).lower(), str(learner).lower()
    table = E.PAIRWISE_LOSSES if pairwise else E.POINTWISE_LOSSES
    if loss not in table:
        raise Exception("please choose a suitable loss function")        # learner.py:28,40
    if learner != "adam" and learner not in E.ROW_OPTIMIZERS:
        raise ValueError("please select a suitable optimizer")           # learner.py:15
    return loss, learner, table[loss]


def slot_init(learner, accumulator=1e-8):
    """(what TF creates the first slot with, None: the learner has no slot; whether there is a second slot, which starts
    at zero) — adam: m, v; adagrad: the accumulator (learner.py:6 passes 1e-8; `accumulator` for a model that builds
    its own tf.train.AdagradOptimizer, whose default is 0.1); rmsprop: rms, its unused momentum; momentum: the
    accumulator"""
    return {"adam": 0.0, "gd": None, "adagrad": accumulator, "rmsprop": 1.0, "momentum": 0.0}[learner], \
        learner in ("adam", "rmsprop")


class RowLearner:
    """One learner of learner.py for the variables of one engine: `adam_state` is the engine's E.AdamState (the engine
    advances it, once per step); `momentum` is MomentumOptimizer's, for the rows and the dense variables alike."""

    def __init__(self, learner, lr, momentum, adam_state, accumulator=1e-8):
        self.learner, self.lr, self.momentum, self.adam = learner, float(lr), float(momentum), adam_state
        self.first, self.two = slot_init(learner, accumulator)
        self.dense = None if learner == "adam" else E.DenseLearner(learner, lr, momentum)

    def slots(self, var):
        """(s0, s1) of `var`: tensors of its shape at TF's initial values, None where the learner has no such slot"""
        return (None if self.first is None else torch.full_like(var, self.first),
                torch.zeros_like(var) if self.two else None)

    def flag(self, n_rows, device):
        """the row flags of a table of n_rows: uint8 zeros; None for Adam, which sweeps every row"""
        return None if self.learner == "adam" else torch.zeros(n_rows, dtype=torch.uint8, device=device)

    def apply(self, var, s0, s1, grad, flag):
        """the sparse application on one table ([rows, d], or [rows] taken as [rows, 1]); the gradient (the flagged
        rows of it, and the flags) is zero again afterwards"""
        if self.learner == "adam":
            E.adam_sparse(var, s0, s1, grad, self.adam)
            return
        if var.dim() == 1:
            var, s0, s1, grad = (None if t is None else t.view(-1, 1) for t in (var, s0, s1, grad))
        if self.learner == "rmsprop":          # tf.train.RMSPropOptimizer(lr): decay 0.9, momentum 0, epsilon 1e-10
            E.optimizer_rows("rmsprop", var, s0, s1, grad, flag, self.lr, 0.9, 0.0, 1e-10)
        elif self.learner == "momentum":
            E.optimizer_rows("momentum", var, s0, None, grad, flag, self.lr, self.momentum)
        else:
            E.optimizer_rows(self.learner, var, s0, None, grad, flag, self.lr)

    def apply_dense(self, tensors, clear_grad):
        """the dense application on (var, s0, s1, grad) tuples; clear_grad: zero the gradients afterwards"""
        if self.dense is None:
            for var, s0, s1, grad in tensors:
                E.adam_dense(var, s0, s1, grad, self.adam, clear_grad=clear_grad)
        elif tensors:
            self.dense.apply([t + (clear_grad,) for t in tensors])


def addr(t):
    """the address of an optional tensor for an argument struct (None: a null pointer)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def f32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32)


def as_ids(x, device, numel=None, what="expected {want} ids, got {n}"):
    """host array or tensor -> contiguous int32 tensor on `device`; numel: the number of entries it must hold, else
    ValueError(what.format(n=the number found, want=numel))"""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32))
    x = x.to(device, torch.int32).contiguous()
    if numel is not None and x.numel() != numel:
        raise ValueError(what.format(n=x.numel(), want=numel))
    return x


class ScoreCache:
    """the scoring GEMM of an engine's score(): made for the largest user count seen, re-prepared for the item side of
    each call"""

    def __init__(self):
        self._gemm = None

    def score(self, P, Q, n_items):
        """[n, n_items]: the rows of P [n, k] against the rows of Q [I, k]"""
        n = int(P.shape[0])
        if self._gemm is None or self._gemm.max_rows < n:
            self._gemm = E.score_gemm_for(Q, max(n, 1))
        else:
            self._gemm.prepare(Q)
        return self._gemm(P, None)[:, :n_items]
