"""GRU4RecPlus on the HIP engine: the graph of model/sequential_recommender/GRU4RecPlus.py:122-151, one
`sess.run([update_opt, final_state])` per step (csrc/gru4recplus.hip).  Everything but the step is GRU4Rec's
(neurec_amd/gru4rec.py): the tables, the optimiser forms (E_in, Q and b: Adam's sparse form; the cells: ApplyAdam), the
recurrent states in HBM, `advance`, the users' final states and predict() — `_get_user_embeddings` and `predict` of the
two reference classes are the same computation.

The step's own: Y holds B + n_sample items, the positives first (the positive of row i is column i) and then the
negatives every row shares; the loss is `bpr_max` or `top1_max`, a softmax over the row's negatives weighting the
pairwise terms (GRU4RecPlus.py:91-120), with `bpr_reg` on the weighted squares of the negatives' scores.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import Gru4recplusStepArgs, call
from .engine import _ptr, _stream
from .row_learner import as_ids
from .gru4rec import _CELL, FINAL_ACTS, HIDDEN_ACTS, MAX_BATCH, GRU4RecEngine

MAX_SAMPLE = 8192             # NRHIP_GRU4RECPLUS_MAX_SAMPLE
LOSSES = {"top1_max": 0, "bpr_max": 1}


class GRU4RecPlusEngine(GRU4RecEngine):
    """GRU4RecEngine with `n_sample` shared negatives per step: `gradients(X, Y, loss_out)` takes
    len(Y) == len(X) + n_sample, `step` and `run_schedule` take Y [S, B + n_sample]."""

    def __init__(self, E_in, Q, b, cells, lr, reg, max_batch, loss="bpr_max", hidden_act="tanh", final_act="linear",
                 bpr_reg=1.0, n_sample=0):
        if hidden_act not in HIDDEN_ACTS:
            raise ValueError("There is not hidden_act named '%s'." % hidden_act)       # GRU4RecPlus.py:37
        if final_act not in FINAL_ACTS:
            raise ValueError("There is not final_act named '%s'." % final_act)         # GRU4RecPlus.py:47
        if loss not in LOSSES:
            raise ValueError("There is not loss named '%s'." % loss)                   # GRU4RecPlus.py:54
        n_sample, max_batch = int(n_sample), int(max_batch)
        if not 0 <= n_sample <= MAX_SAMPLE:
            raise NotImplementedError("GRU4RecPlus: n_sample=%d is not supported (0 to %d)" % (n_sample, MAX_SAMPLE))
        if max_batch == 1 and n_sample == 0:
            raise NotImplementedError("GRU4RecPlus: batch_size + n_sample = %d: a row needs at least one negative "
                                      "(the reference divides 0 by 0)" % (max_batch + n_sample))
        # the base class knows GRU4Rec's loss names only; this model's own is set right after
        GRU4RecEngine.__init__(self, E_in, Q, b, cells, lr, reg, max_batch, loss="top1", hidden_act=hidden_act,
                               final_act=final_act)
        self.loss, self.bpr_reg, self.n_sample = loss, float(bpr_reg), n_sample
        dev = self.E_in.device
        self._keys = torch.empty(2 * max_batch + n_sample, dtype=torch.int64, device=dev)
        floats = C.c_size_t(0)
        call("nrhip_gru4recplus_workspace_floats", self.n_layers, self._widths, max_batch, n_sample, C.byref(floats))
        self._ws = torch.empty(max(int(floats.value), 1), dtype=torch.float32, device=dev)

    def gradients(self, X, Y, loss_out):
        """the C call alone, as GRU4RecEngine.gradients; Y: the B positives, then the n_sample negatives"""
        B = int(X.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if B == 0:
            loss_out.zero_()
            return
        if Y.numel() != B + self.n_sample:
            raise ValueError("Y must hold len(X) + n_sample items")
        a = Gru4recplusStepArgs()
        a.Ein, a.Q, a.b = _ptr(self.E_in), _ptr(self.Q), _ptr(self.b)
        a.w = self._weights()
        a.G_Ein, a.G_Q, a.G_b = _ptr(self.G["E_in"]), _ptr(self.G["Q"]), _ptr(self.G["b"])
        for l in range(self.n_layers):
            for name in _CELL:
                getattr(a, "G_" + name)[l] = self.G["%s%d" % (name, l)].data_ptr()
            a.state[l], a.h_new[l] = self.states[l].data_ptr(), self.h_new[l].data_ptr()
        a.X, a.Y = _ptr(X, torch.int32), _ptr(Y, torch.int32)
        a.keys, a.ws, a.loss2 = _ptr(self._keys), _ptr(self._ws), _ptr(loss_out, torch.float32)
        a.n_items, a.batch, a.n_sample = self.n_items, B, self.n_sample
        a.final_act, a.loss_kind = FINAL_ACTS[self.final_act], LOSSES[self.loss]
        a.reg, a.bpr_reg = self.reg, self.bpr_reg
        call("nrhip_gru4recplus_step", C.byref(a), _stream())

    def run_schedule(self, X, Y, reset, losses):
        """a whole epoch: X int32 [S, B], Y int32 [S, B + n_sample], reset uint8 [S, B], losses float32 [S, 2] on the
        device, or host arrays that are uploaded once; no host round trip between the steps.  The items of host arrays
        are checked against the table here (GRU4RecEngine.run_schedule)."""
        for name, a in (("X", X), ("Y", Y)):
            if not isinstance(a, torch.Tensor) and np.size(a) and (np.min(a) < 0 or np.max(a) >= self.n_items):
                raise ValueError("GRU4RecPlus: %s holds an item outside [0, %d)" % (name, self.n_items))
        dev = self.E_in.device
        up = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        X, Y = as_ids(X, dev), as_ids(Y, dev)
        reset = up(reset).to(dev, torch.uint8).contiguous()
        if X.dim() != 2 or Y.dim() != 2 or Y.shape[0] != X.shape[0] or Y.shape[1] != X.shape[1] + self.n_sample or \
                X.shape != reset.shape or losses.shape[0] < X.shape[0]:
            raise ValueError("X and reset must be [steps, batch], Y [steps, batch + n_sample], losses [steps, 2]")
        for s in range(int(X.shape[0])):
            self.step(X[s], Y[s], losses[s], reset[s])
        return losses
