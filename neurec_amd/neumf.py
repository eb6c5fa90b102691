"""NeuMF and MLP on the HIP engine: the graph of model/general_recommender/NeuMF.py:69-100 (MLP.py is the same model
without the GMF branch), one `sess.run((loss, optimizer))` per step in pointwise mode, and predict() (csrc/neumf.hip).

Variables in creation order: mf_embedding_user [U, d], mf_embedding_item [I, d] (NeuMF only), mlp_embedding_user [U, e],
mlp_embedding_item [I, e] with e = int(layers[0] / 2), then per layer k the `tf.layers.dense` pair kernel<k> [in_k,
layers[k]] and bias<k> [layers[k]]; in_0 = 2 e (layers[0] only when that is even), in_k = layers[k - 1].

    y(u, i) = sum(mf_user[u] * mf_item[i]) + sum(h_last),  h_k = relu(h_{k-1} kernel_k + bias_k),  h_{-1} = [m_u | n_i]

There is no learned output layer and no sigmoid.  `cross_entropy` is tf.losses.sigmoid_cross_entropy, the MEAN over the
batch; `square` is a sum.  The regulariser reg_mf l2_loss(p_u, q_i) + reg_mlp l2_loss(m_u, n_i) is taken on the gathered
rows: a row the batch holds twice counts twice.

Optimiser forms, as TF-1.12 picks them: the four tables are read through embedding_lookup only — IndexedSlices, the
sparse application (neurec_amd/row_learner.py: Adam sweeps every row, the other learners move the rows the step
flagged); kernels and biases are dense variables — the dense Apply* kernels.
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from ._lib import NeumfStepArgs, NeumfWeights, call
from .engine import _ptr, _stream
from .row_learner import RowLearner, addr, as_ids, check_loss_learner, f32

MAX_WIDTH = 128               # NRHIP_NEUMF_MAX_WIDTH
MAX_LAYERS = 4                # NRHIP_NEUMF_MAX_LAYERS
MAX_BATCH = 4096              # NRHIP_NEUMF_MAX_BATCH
MF_TABLES = ("mf_embedding_user", "mf_embedding_item")
MLP_TABLES = ("mlp_embedding_user", "mlp_embedding_item")
# table -> its field in nrhip_neumf_weights (the gradient's and the flag's in nrhip_neumf_step_args: G_ / flag_ in front)
FIELDS = {"mf_embedding_user": "mf_user", "mf_embedding_item": "mf_item", "mlp_embedding_user": "mlp_user",
          "mlp_embedding_item": "mlp_item"}


def check_shape(name, embedding_size, layers):
    """the refusals of a shape the kernels were not built for; embedding_size 0 is MLP"""
    layers = [int(x) for x in layers]
    if not 1 <= len(layers) <= MAX_LAYERS:
        raise NotImplementedError("%s: layers=%r is not supported (1 to %d layers)" % (name, layers, MAX_LAYERS))
    for k, w in enumerate(layers):
        if not 1 <= w <= MAX_WIDTH:
            raise NotImplementedError("%s: layers[%d]=%d is not supported (1 to %d)" % (name, k, w, MAX_WIDTH))
    if not 0 <= int(embedding_size) <= MAX_WIDTH:
        raise NotImplementedError("%s: embedding_size=%d is not supported (%d to %d)" % (
            name, embedding_size, 0 if name == "MLP" else 1, MAX_WIDTH))
    return layers


def table_names(n_layers, with_mf=True):
    out = list(MF_TABLES if with_mf else ()) + list(MLP_TABLES)
    for k in range(n_layers):
        out += ["kernel%d" % k, "bias%d" % k]
    return out


def layer_inputs(layers):
    """in_k of every layer: 2 (layers[0] // 2), then the width below"""
    return [2 * (int(layers[0]) // 2)] + [int(w) for w in layers[:-1]]


class NeuMFEngine:
    """Tables, dense variables, optimiser slots and gradient buffers in HBM.

    `variables`: {name: array} of table_names(len(layers), with_mf); without the mf_* tables the engine is MLP.
    `step(users, items, labels, loss_out)`: one batch of the pointwise instance stream — gradients, then the learner.
    `forward(users, items)` -> the pairs' scores; `score(users)` -> [n, I] on the device."""

    def __init__(self, variables, layers, lr, reg_mf, reg_mlp, max_batch, loss="cross_entropy", learner="adam",
                 momentum=0.9, name=None):
        with_mf = "mf_embedding_user" in variables
        self.name = name or ("NeuMF" if with_mf else "MLP")
        loss, learner, self.loss_kind = check_loss_learner(loss, learner, False)
        mlp_user, mlp_item = f32(variables["mlp_embedding_user"]), f32(variables["mlp_embedding_item"])
        if mlp_user.dim() != 2 or mlp_item.dim() != 2:
            raise ValueError("mlp_embedding_user must be [num_users, layers[0] // 2], mlp_embedding_item [num_items, "
                             "layers[0] // 2]")
        U, I = int(mlp_user.shape[0]), int(mlp_item.shape[0])
        d = int(f32(variables["mf_embedding_user"]).shape[1]) if with_mf else 0
        layers = check_shape(self.name, d, layers)
        if with_mf and d < 1:
            raise NotImplementedError("%s: embedding_size=%d is not supported (1 to %d)" % (self.name, d, MAX_WIDTH))
        max_batch = int(max_batch)
        if max_batch < 1:
            raise ValueError("max_batch must be at least 1")
        if max_batch > MAX_BATCH:
            raise NotImplementedError("%s: batch_size=%d is not supported (1 to %d)" % (self.name, max_batch, MAX_BATCH))
        if U + I >= 1 << 31:
            raise NotImplementedError("%s: num_users + num_items = %d is not supported (below 2^31)" % (self.name, U + I))
        e, ins = layers[0] // 2, layer_inputs(layers)
        shapes = {"mf_embedding_user": (U, d), "mf_embedding_item": (I, d), "mlp_embedding_user": (U, e),
                  "mlp_embedding_item": (I, e)}
        for k, w in enumerate(layers):
            shapes["kernel%d" % k], shapes["bias%d" % k] = (ins[k], w), (w,)
        names = table_names(len(layers), with_mf)
        if sorted(variables) != sorted(names):
            raise ValueError("variables must be %s" % ", ".join(names))
        dev = E.require_gpu()
        self.T = {}
        for n in names:
            t = f32(variables[n])
            if t.numel() != int(np.prod(shapes[n])):
                raise ValueError("%s holds %d values, want %s" % (n, t.numel(), "x".join(map(str, shapes[n]))))
            self.T[n] = t.reshape(shapes[n]).contiguous().to(dev)
        self.n_users, self.n_items, self.d, self.e, self.layers = U, I, d, e, layers
        self.rows = [n for n in names if n in FIELDS]
        self.dense = [n for n in names if n not in FIELDS]
        self.max_batch, self.loss, self.learner = max_batch, loss, learner
        self.lr, self.reg_mf, self.reg_mlp = float(lr), float(reg_mf), float(reg_mlp)
        self.adam = E.AdamState(lr)
        self.opt = RowLearner(learner, lr, momentum, self.adam)
        self.G = {k: torch.zeros_like(t) for k, t in self.T.items()}
        slots = {k: self.opt.slots(t) for k, t in self.T.items()}
        self.s0, self.s1 = ({k: s[i] for k, s in slots.items()} for i in (0, 1))
        self.flag = {k: self.opt.flag(self.T[k].shape[0], dev) for k in self.rows}
        self._keys = torch.empty(2 * max_batch, dtype=torch.int64, device=dev)
        self._ws = torch.empty(max(self.workspace_floats(max_batch), 1), dtype=torch.float32, device=dev)
        self._score_ws = None
        self.t = 0

    def tables(self):
        """{name: tensor} of every variable, in creation order"""
        return dict(self.T)

    def _weights(self):
        w = NeumfWeights()
        for n in self.rows:
            setattr(w, FIELDS[n], addr(self.T[n]) if self.T[n].numel() else None)
        for k, width in enumerate(self.layers):
            w.kernel[k] = self.T["kernel%d" % k].data_ptr() if self.T["kernel%d" % k].numel() else None
            w.bias[k] = self.T["bias%d" % k].data_ptr()
            w.width[k] = width
        w.n_users, w.n_items, w.d, w.n_layers = self.n_users, self.n_items, self.d, len(self.layers)
        return w

    def workspace_floats(self, batch=None):
        """the floats of work space a step of `batch` instances takes (max_batch when None)"""
        floats = C.c_size_t(0)
        w = self._weights()
        call("nrhip_neumf_workspace_floats", C.byref(w), self.max_batch if batch is None else int(batch),
             C.byref(floats))
        return int(floats.value)

    # ------------------------------------------------------------------ inputs
    def _check_host(self, what, a, hi):
        """host arrays only: ids in [0, hi)"""
        if not isinstance(a, torch.Tensor) and np.size(a) and (np.min(a) < 0 or np.max(a) >= hi):
            raise ValueError("%s: %s holds an id outside [0, %d)" % (self.name, what, hi))

    def _pairs(self, users, items):
        self._check_host("users", users, self.n_users)
        self._check_host("items", items, self.n_items)
        dev = self.T["mlp_embedding_user"].device
        users, items = as_ids(users, dev), as_ids(items, dev)
        if users.dim() != 1 or items.dim() != 1 or users.numel() != items.numel():
            raise ValueError("users and items must be [batch] each")
        return users, items

    # ------------------------------------------------------------------ training
    def gradients(self, users, items, labels, loss_out):
        """the C call alone: loss_out (2 floats on the device: data term, regulariser term), the dense gradients and the
        batch's rows of the tables' gradients (and the row flags); no variable moves.  Host arrays are checked for ids
        outside their tables.  An empty batch is no work: nothing is launched and loss_out is set to zero."""
        users, items = self._pairs(users, items)
        B = int(users.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if not isinstance(labels, torch.Tensor):
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float32))
        labels = labels.to(users.device, torch.float32).contiguous()
        if labels.numel() != B:
            raise ValueError("users, items and labels must have the same length")
        if B == 0:
            loss_out.zero_()
            return
        a = NeumfStepArgs()
        a.w = self._weights()
        for n in self.rows:
            if self.T[n].numel():
                setattr(a, "G_" + FIELDS[n], _ptr(self.G[n]))
                setattr(a, "flag_" + FIELDS[n], addr(self.flag[n]))
        for k in range(len(self.layers)):
            a.G_kernel[k] = self.G["kernel%d" % k].data_ptr() if self.G["kernel%d" % k].numel() else None
            a.G_bias[k] = self.G["bias%d" % k].data_ptr()
        a.users, a.items, a.labels = _ptr(users, torch.int32), _ptr(items, torch.int32), _ptr(labels, torch.float32)
        a.keys, a.ws, a.loss2 = _ptr(self._keys), _ptr(self._ws), _ptr(loss_out, torch.float32)
        a.batch, a.loss_kind, a.reg_mf, a.reg_mlp = B, self.loss_kind, self.reg_mf, self.reg_mlp
        call("nrhip_neumf_step", C.byref(a), _stream())

    def apply(self):
        """the tables in the learner's sparse form, kernels and biases in its dense form; the gradient buffers (and the
        row flags) are zero again afterwards"""
        for n in self.rows:
            if self.T[n].numel():
                self.opt.apply(self.T[n], self.s0[n], self.s1[n], self.G[n], self.flag[n])
        dense = [(self.T[n], self.s0[n], self.s1[n], self.G[n]) for n in self.dense if self.T[n].numel()]
        if self.learner == "adam":                         # ApplyAdam on every kernel and bias in one launch
            E.adam_dense_multi([t + (True,) for t in dense], self.adam)
        else:
            self.opt.apply_dense(dense, True)
        self.adam.advance()
        self.t += 1

    def step(self, users, items, labels, loss_out):
        """gradients, then the learner; an empty batch moves nothing"""
        self.gradients(users, items, labels, loss_out)
        if int(np.shape(users)[0]) == 0:
            return
        self.apply()

    # ------------------------------------------------------------------ scoring
    def forward(self, users, items):
        """y(users[k], items[k]) [n] float32 on the device, through the step's forward path"""
        users, items = self._pairs(users, items)
        n = int(users.numel())
        out = torch.empty(n, dtype=torch.float32, device=users.device)
        if n:
            w = self._weights()
            call("nrhip_neumf_forward", C.byref(w), _ptr(users, torch.int32), _ptr(items, torch.int32), n, _ptr(out),
                 _stream())
        return out

    def score(self, users, out=None):
        """S [n, I] float32 on the device: predict() of NeuMF.py:165-168 for `users`, every item.  out: a float32
        device tensor whose leading [n, I] block is written (rows of any stride), the rest left as it is"""
        self._check_host("users", users, self.n_users)
        users = as_ids(users, self.T["mlp_embedding_user"].device).reshape(-1)
        n, I = int(users.numel()), self.n_items
        if out is None:
            out = torch.empty((n, I), dtype=torch.float32, device=users.device)
        elif out.dim() != 2 or out.shape[0] < n or out.shape[1] < I or out.stride(1) != 1 or out.dtype != torch.float32:
            raise ValueError("out must be a float32 [>= n, >= num_items] tensor with unit column stride")
        if n == 0 or I == 0:
            return out[:n, :I]
        w = self._weights()
        floats = C.c_size_t(0)
        call("nrhip_neumf_scores_workspace_floats", C.byref(w), n, C.byref(floats))
        if self._score_ws is None or self._score_ws.numel() < floats.value:
            self._score_ws = None
            self._score_ws = torch.empty(int(floats.value), dtype=torch.float32, device=users.device)
        call("nrhip_neumf_scores", C.byref(w), _ptr(users, torch.int32), n, _ptr(self._score_ws),
             C.c_void_p(out.data_ptr()), int(out.stride(0)), _stream())
        return out[:n, :I]
