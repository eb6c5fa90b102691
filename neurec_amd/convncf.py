"""ConvNCF on the HIP engine: the graph of model/general_recommender/ConvNCF.py:87-145, one `sess.run((self.loss,
self.optimizer))` per step, and predict() (csrc/convncf.hip).

Variables in creation order: embedding_P [U, d], embedding_Q [I, d], then per layer k the pair kernel<k> [2, 2, c_in,
net_channel[k]] and bias<k> [net_channel[k]] (c_in = 1 for the first layer), then W [net_channel[-1], 1] and b [1].

    output(u, i) = a_L W + b,  a_k = tanh(conv2d(a_{k-1}, kernel_k, strides 2, SAME) + bias_k),  a_0 = p_u (x) q_i [d, d, 1]

with d == 2^L, so a_L has one position; no sigmoid.  loss = pairwise_loss(output(u, pos) - output(u, neg)), summed;
opt_loss adds regs[0] l2_loss(p1, q2, q1) on the gathered rows (the user row once per triplet), regs[1] l2_loss(W, b) and
regs[2] (sum_k l2_loss(kernel_k, bias_k) + l2_loss(W, b)).

Learner: two tf.train.AdagradOptimizer, lr_embed for the tables and lr_net for everything else, their accumulators
starting at 0.1 (TF's default, not the 1e-8 of util/learner.py).  The tables are read through embedding_lookup only —
the sparse application on the rows the step flagged; kernels, biases, W and b take the dense Apply kernel.
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from ._lib import ConvncfStepArgs, ConvncfWeights, call
from .engine import _ptr, _stream
from .row_learner import RowLearner, addr, as_ids, f32

MAX_LAYERS = 6                # NRHIP_CONVNCF_MAX_LAYERS
MAX_CHANNELS = 32             # NRHIP_CONVNCF_MAX_CHANNELS
MAX_BATCH = 4096              # NRHIP_CONVNCF_MAX_BATCH
ACCUMULATOR = 0.1             # tf.train.AdagradOptimizer(initial_accumulator_value=0.1)
TABLES = ("embedding_P", "embedding_Q")


def check_shape(embedding_size, net_channel):
    """the refusals of a shape the kernels were not built for"""
    channels = [int(c) for c in net_channel]
    if not 1 <= len(channels) <= MAX_LAYERS:
        raise NotImplementedError("ConvNCF: net_channel=%r is not supported (1 to %d layers)" % (channels, MAX_LAYERS))
    for k, c in enumerate(channels):
        if not 1 <= c <= MAX_CHANNELS:
            raise NotImplementedError("ConvNCF: net_channel[%d]=%d is not supported (1 to %d)" % (k, c, MAX_CHANNELS))
    if int(embedding_size) != 1 << len(channels):
        raise NotImplementedError("ConvNCF: embedding_size=%d is not supported with %d layers in net_channel (the graph "
                                  "gives one value per pair only for embedding_size == 2**len(net_channel) = %d; 2 to %d)"
                                  % (embedding_size, len(channels), 1 << len(channels), 1 << MAX_LAYERS))
    return channels


def table_names(n_layers):
    out = list(TABLES)
    for k in range(n_layers):
        out += ["kernel%d" % k, "bias%d" % k]
    return out + ["W", "b"]


class ConvNCFEngine:
    """Tables, dense variables, Adagrad accumulators and gradient buffers in HBM.

    `variables`: {name: array} of table_names(len(net_channel)).
    `step(users, pos, neg, loss_out)`: one batch of triplets — gradients, then the two Adagrad applications.
    `forward(users, items)` -> the pairs' outputs; `score(users)` -> [n, I] on the device."""

    def __init__(self, variables, net_channel, lr_embed, lr_net, regs, max_batch, loss="bpr"):
        self.name = "ConvNCF"
        loss = str(loss).lower()
        if loss not in E.PAIRWISE_LOSSES:
            raise Exception("please choose a suitable loss function")        # learner.py:28
        self.loss, self.loss_kind = loss, E.PAIRWISE_LOSSES[loss]
        P, Q = f32(variables["embedding_P"]), f32(variables["embedding_Q"])
        if P.dim() != 2 or Q.dim() != 2 or P.shape[1] != Q.shape[1]:
            raise ValueError("embedding_P must be [num_users, embedding_size], embedding_Q [num_items, embedding_size]")
        U, I, d = int(P.shape[0]), int(Q.shape[0]), int(P.shape[1])
        channels = check_shape(d, net_channel)
        max_batch = int(max_batch)
        if max_batch < 1:
            raise ValueError("max_batch must be at least 1")
        if max_batch > MAX_BATCH:
            raise NotImplementedError("ConvNCF: batch_size=%d is not supported (1 to %d)" % (max_batch, MAX_BATCH))
        if U + I >= 1 << 31:
            raise NotImplementedError("ConvNCF: num_users + num_items = %d is not supported (below 2^31)" % (U + I))
        regs = [float(r) for r in regs]
        if len(regs) != 3:
            raise ValueError("regs must hold three values")
        shapes = {"embedding_P": (U, d), "embedding_Q": (I, d), "W": (channels[-1], 1), "b": (1,)}
        c_in = 1
        for k, c in enumerate(channels):
            shapes["kernel%d" % k], shapes["bias%d" % k] = (2, 2, c_in, c), (c,)
            c_in = c
        names = table_names(len(channels))
        if sorted(variables) != sorted(names):
            raise ValueError("variables must be %s" % ", ".join(names))
        dev = E.require_gpu()
        self.T = {}
        for n in names:
            t = f32(variables[n])
            if t.numel() != int(np.prod(shapes[n])):
                raise ValueError("%s holds %d values, want %s" % (n, t.numel(), "x".join(map(str, shapes[n]))))
            self.T[n] = t.reshape(shapes[n]).contiguous().to(dev)
        self.n_users, self.n_items, self.d, self.channels = U, I, d, channels
        self.rows = list(TABLES)
        self.dense = [n for n in names if n not in TABLES]
        self.max_batch, self.regs = max_batch, regs
        self.lr_embed, self.lr_net = float(lr_embed), float(lr_net)
        self.opt = RowLearner("adagrad", self.lr_embed, 0.0, None, accumulator=ACCUMULATOR)
        self.opt_net = E.DenseLearner("adagrad", self.lr_net)
        self.G = {k: torch.zeros_like(t) for k, t in self.T.items()}
        self.acc = {k: self.opt.slots(t)[0] for k, t in self.T.items()}
        self.flag = {k: self.opt.flag(self.T[k].shape[0], dev) for k in self.rows}
        self._keys = torch.empty(4 * max_batch, dtype=torch.int64, device=dev)
        self._ws = torch.empty(max(self.workspace_floats(max_batch), 1), dtype=torch.float32, device=dev)
        self.t = 0

    def tables(self):
        """{name: tensor} of every variable, in creation order"""
        return dict(self.T)

    def _weights(self):
        w = ConvncfWeights()
        w.P, w.Q = addr(self.T["embedding_P"]), addr(self.T["embedding_Q"])
        for k, c in enumerate(self.channels):
            w.kernel[k] = self.T["kernel%d" % k].data_ptr()
            w.bias[k] = self.T["bias%d" % k].data_ptr()
            w.channel[k] = c
        w.W, w.b = addr(self.T["W"]), addr(self.T["b"])
        w.n_users, w.n_items, w.d, w.n_layers = self.n_users, self.n_items, self.d, len(self.channels)
        return w

    def workspace_floats(self, batch=None):
        """the floats of work space a step of `batch` triplets takes (max_batch when None)"""
        floats = C.c_size_t(0)
        w = self._weights()
        call("nrhip_convncf_workspace_floats", C.byref(w), self.max_batch if batch is None else int(batch),
             C.byref(floats))
        return int(floats.value)

    # ------------------------------------------------------------------ inputs
    def _check_host(self, what, a, hi):
        """host arrays only: ids in [0, hi)"""
        if not isinstance(a, torch.Tensor) and np.size(a) and (np.min(a) < 0 or np.max(a) >= hi):
            raise ValueError("ConvNCF: %s holds an id outside [0, %d)" % (what, hi))

    def _ids(self, what, a, hi):
        self._check_host(what, a, hi)
        a = as_ids(a, self.T["embedding_P"].device)
        if a.dim() != 1:
            raise ValueError("%s must be [batch]" % what)
        return a

    # ------------------------------------------------------------------ training
    def gradients(self, users, pos, neg, loss_out):
        """the C call alone: loss_out (2 floats on the device: self.loss, the regs[0] term), the dense gradients and the
        batch's rows of the tables' gradients (and the row flags); no variable moves.  Host arrays are checked for ids
        outside their tables.  An empty batch is no work: nothing is launched and no buffer, loss_out included, is touched."""
        users = self._ids("users", users, self.n_users)
        pos, neg = self._ids("pos", pos, self.n_items), self._ids("neg", neg, self.n_items)
        B = int(users.numel())
        if pos.numel() != B or neg.numel() != B:
            raise ValueError("users, pos and neg must have the same length")
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if B == 0:
            return
        a = ConvncfStepArgs()
        a.w = self._weights()
        a.G_P, a.G_Q = _ptr(self.G["embedding_P"]), _ptr(self.G["embedding_Q"])
        a.flag_P, a.flag_Q = addr(self.flag["embedding_P"]), addr(self.flag["embedding_Q"])
        for k in range(len(self.channels)):
            a.G_kernel[k] = self.G["kernel%d" % k].data_ptr()
            a.G_bias[k] = self.G["bias%d" % k].data_ptr()
        a.G_W, a.G_b = _ptr(self.G["W"]), _ptr(self.G["b"])
        a.users, a.pos, a.neg = _ptr(users, torch.int32), _ptr(pos, torch.int32), _ptr(neg, torch.int32)
        a.keys, a.ws, a.loss2 = _ptr(self._keys), _ptr(self._ws), _ptr(loss_out, torch.float32)
        a.batch, a.loss_kind = B, self.loss_kind
        a.reg_embed, a.reg_head, a.reg_net = self.regs
        call("nrhip_convncf_step", C.byref(a), _stream())

    def apply(self):
        """Adagrad: the tables' flagged rows at lr_embed, everything else in the dense form at lr_net; the gradient
        buffers (and the row flags) are zero again afterwards"""
        for n in self.rows:
            self.opt.apply(self.T[n], self.acc[n], None, self.G[n], self.flag[n])
        self.opt_net.apply([(self.T[n].view(-1), self.acc[n].view(-1), None, self.G[n].view(-1), True)
                            for n in self.dense])
        self.t += 1

    def step(self, users, pos, neg, loss_out):
        """gradients, then the learner; an empty batch moves nothing"""
        self.gradients(users, pos, neg, loss_out)
        if int(np.shape(users)[0]) == 0:
            return
        self.apply()

    # ------------------------------------------------------------------ scoring
    def forward(self, users, items):
        """output(users[k], items[k]) [n] float32 on the device, through the step's forward path"""
        users, items = self._ids("users", users, self.n_users), self._ids("items", items, self.n_items)
        if users.numel() != items.numel():
            raise ValueError("users and items must be [batch] each")
        n = int(users.numel())
        out = torch.empty(n, dtype=torch.float32, device=users.device)
        if n:
            w = self._weights()
            call("nrhip_convncf_pairs", C.byref(w), _ptr(users, torch.int32), _ptr(items, torch.int32), n, _ptr(out),
                 _stream())
        return out

    def score(self, users, out=None):
        """S [n, I] float32 on the device: predict() of ConvNCF.py:196-199 for `users`, every item.  out: a float32
        device tensor whose leading [n, I] block is written (rows of any stride), the rest left as it is"""
        users = self._ids("users", np.reshape(users, -1) if not isinstance(users, torch.Tensor) else users.reshape(-1),
                          self.n_users)
        n, I = int(users.numel()), self.n_items
        if out is None:
            out = torch.empty((n, I), dtype=torch.float32, device=users.device)
        elif out.dim() != 2 or out.shape[0] < n or out.shape[1] < I or out.stride(1) != 1 or out.dtype != torch.float32:
            raise ValueError("out must be a float32 [>= n, >= num_items] tensor with unit column stride")
        if n == 0 or I == 0:
            return out[:n, :I]
        w = self._weights()
        call("nrhip_convncf_scores", C.byref(w), _ptr(users, torch.int32), n, C.c_void_p(out.data_ptr()),
             int(out.stride(0)), _stream())
        return out[:n, :I]
