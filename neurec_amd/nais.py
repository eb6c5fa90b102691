"""NAIS on the HIP engine: the graph of NAIS.py:96-176 and one `sess.run((loss, optimizer))` per step, and predict()
(csrc/nais.hip).

NAIS is FISM with the plain sum over the history replaced by an attention-weighted sum whose weights depend on the
target item: A_j = exp(h . act(x_j W + b)) / (sum of them)^beta, x_j = c1[h_j] (.) Q[i] (algorithm 0) or the two
concatenated (algorithm 1).  As in neurec_amd/fism.py a wave walks the user's CSR row: neither the padded id matrix nor
a gathered [B, Lmax, d] block exist.  The score is not an inner product of user and item factors, so predict() has a
kernel of its own: e(i, h) does not depend on the user, and a block of users shares the (target, history item) terms.

Optimiser forms, as TF-1.12 picks them: `c1` is read through tf.concat and W, b, h are dense variables — the dense
Apply* kernels; `embedding_Q` and `bias` are read through embedding_lookup — the sparse application.
`c1_application="rows"` gives c1 the sparse application as well.

`attention_mask="reference"` (default) reproduces the reference's mask, sequence_mask(num_idx) with num_idx = |H| + 1:
an instance whose history is shorter than the longest of its side of the batch has one zero row inside the mask, whose
exp() joins the softmax's sum.  `attention_mask="history"` is the paper's softmax over exactly H (what predict computes).
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import torch

from . import engine as E
from ._lib import NaisScoresArgs, NaisStepArgs, call
from .engine import _ptr, _stream

MAX_D = 128                   # NRHIP_NAIS_MAX_D
MAX_W = 64                    # NRHIP_NAIS_MAX_W
ACTIVATIONS = {0: "relu", 1: "sigmoid", 2: "tanh"}
SCORE_WS_BYTES = 256 << 20    # the two [history items, tile] buffers of score()


C1_PATH = "walk"              # how G_c1 is summed: "walk" or "sort" (DESIGN 6e has the A/B)
PAIR_KERNEL = "mfma"          # score()'s pair kernel where both exist (algorithm 0, d <= 16, w <= 16): "valu" or "mfma"


def _addr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def activation_code(activation):
    """NAIS.py:158-163 compares conf["activation"] with the ints 0 / 1 / 2; anything else applies no activation"""
    for k in ACTIVATIONS:
        if type(activation) in (int, np.int32, np.int64) and activation == k:
            return k
    return 3


class NAISEngine:
    """Tables c1 / Q / bias / W / b / h, their optimiser state and gradient buffers in HBM.

    `step(users, items, third, loss_out)`: one batch of the device instance stream, as FISMEngine.step.
    `score(users)` -> [B, I] on the device: predict() on the whole train row."""

    def __init__(self, c1, Q, W, b, train, lr, regs, alpha, beta, max_batch, algorithm=0, activation=None,
                 loss="cross_entropy", pairwise=False, learner="adam", bias=None, h=None, momentum=0.9,
                 attention_mask="reference", c1_application="dense", c1_path=C1_PATH, pair_kernel="auto"):
        loss, learner = str(loss).lower(), str(learner).lower()
        table = E.PAIRWISE_LOSSES if pairwise else E.POINTWISE_LOSSES
        if loss not in table:
            raise Exception("please choose a suitable loss function")        # learner.py:28,40
        if learner != "adam" and learner not in E.ROW_OPTIMIZERS:
            raise ValueError("please select a suitable optimizer")           # learner.py:15
        if c1_application not in ("dense", "rows"):
            raise ValueError("c1_application is 'dense' or 'rows', got %r" % (c1_application,))
        if attention_mask not in ("reference", "history"):
            raise ValueError("attention_mask is 'reference' or 'history', got %r" % (attention_mask,))
        if algorithm not in (0, 1):
            raise ValueError("algorithm is 0 (product) or 1 (concat), got %r" % (algorithm,))
        if not float(beta) >= 0.0:
            raise ValueError("NAIS needs beta >= 0, got %r" % (beta,))
        f32 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
        c1, Q, W = f32(c1), f32(Q), f32(W)
        if c1.dim() != 2 or tuple(c1.shape) != tuple(Q.shape):
            raise ValueError("c1 and embedding_Q must both be [num_items, embedding_size]")
        I, d = c1.shape
        if d < 1 or d > MAX_D:
            raise NotImplementedError("NAIS: embedding_size=%d is not supported (1 to %d)" % (d, MAX_D))
        if W.dim() != 2 or W.shape[0] != (algorithm + 1) * d:
            raise ValueError("W must be [%d, weight_size]" % ((algorithm + 1) * d,))
        w = int(W.shape[1])
        if w < 1 or w > MAX_W:
            raise NotImplementedError("NAIS: weight_size=%d is not supported (1 to %d)" % (w, MAX_W))
        b = f32(b).reshape(-1)
        h = torch.ones(w) if h is None else f32(h).reshape(-1)
        if b.numel() != w or h.numel() != w:
            raise ValueError("b and h must hold weight_size entries")
        M = sp.csr_matrix(train)
        if M.shape[1] != I:
            raise ValueError("train matrix has %d items, the tables %d" % (M.shape[1], I))
        M.sum_duplicates()
        M.sort_indices()                                       # the walk finds an item in a row by bisection
        dev = E.require_gpu()
        self.loss, self.pairwise, self.learner = loss, bool(pairwise), learner
        self.loss_kind = table[loss]
        self.algorithm, self.activation = int(algorithm), activation_code(activation)
        self.reference_mask = attention_mask == "reference"
        self.n_users, self.n_items, self.d, self.w = M.shape[0], I, d, w
        self.csr = E.DeviceCSR.from_scipy(M)
        self.csc = E.DeviceCSR.from_scipy(M.T)                 # item -> its users, ascending
        self.h_deg = np.diff(np.asarray(M.indptr, dtype=np.int64))
        dv = lambda t: t.contiguous().to(dev)
        self.c1, self.Q, self.W, self.b, self.h = dv(c1), dv(Q), dv(W), dv(b), dv(h)
        self.bias = dv(torch.zeros(I) if bias is None else f32(bias))
        self._names = ("c1", "Q", "bias", "W", "b", "h")
        self.G = {k: torch.zeros_like(getattr(self, k)) for k in self._names}
        self.lr, self.momentum, self.alpha, self.beta = float(lr), float(momentum), float(alpha), float(beta)
        self.reg_p, self.reg_q = float(regs[0]), float(regs[1])     # regs[2] is read and never used (NAIS.py:33)
        self.adam = E.AdamState(lr)
        self.dense = E.make_learner(learner, lr)               # the dense variables' learner; None: ApplyAdam
        init = {"adam": 0.0, "gd": None, "adagrad": 1e-8, "rmsprop": 1.0, "momentum": 0.0}[learner]
        two = learner in ("adam", "rmsprop")
        mk = lambda t, v: None if v is None else torch.full_like(t, v)
        self.s0 = {k: mk(getattr(self, k), init) for k in self._names}
        self.s1 = {k: (mk(getattr(self, k), 0.0) if two else None) for k in self._names}
        rows = learner != "adam"
        self.flag_Q = torch.zeros(I, dtype=torch.uint8, device=dev) if rows else None
        self.flag_bias = torch.zeros(I, dtype=torch.uint8, device=dev) if rows else None
        self.c1_rows = c1_application == "rows"
        if c1_path not in ("walk", "sort"):
            raise ValueError("c1_path is 'walk' or 'sort', got %r" % (c1_path,))
        if pair_kernel not in ("auto", "valu", "mfma"):
            raise ValueError("pair_kernel is 'auto', 'valu' or 'mfma', got %r" % (pair_kernel,))
        mfma_ok = algorithm == 0 and d <= 16 and w <= 16
        if pair_kernel == "mfma" and not mfma_ok:
            raise NotImplementedError("NAIS: the matrix-core pair kernel takes algorithm 0 with embedding_size <= 16 "
                                      "and weight_size <= 16")
        self.c1_sort = c1_path == "sort"
        self.mfma = (PAIR_KERNEL if pair_kernel == "auto" else pair_kernel) == "mfma" and mfma_ok
        self.flag_c1 = torch.zeros(I, dtype=torch.uint8, device=dev) if (rows and self.c1_rows) else None
        self.max_batch = int(max_batch)
        N = max(self.max_batch, 1) * (2 if self.pairwise else 1)
        # the ragged [positions, d] buffer holds one row per history position of the BATCH (an instance takes its
        # user's train-row length); it starts at the mean batch's size and grows to what a batch asks (reserve)
        self.d_deg = torch.from_numpy(self.h_deg).to(dev)
        self._need = torch.zeros(2, dtype=torch.int64, device=dev)
        self.row_cap = max(64, int(np.ceil(N * float(self.h_deg.mean() if len(self.h_deg) else 0.0))))
        self._keys = torch.empty(2 * N, dtype=torch.int64, device=dev)
        self._inst = torch.empty(4 * N, dtype=torch.int32, device=dev)
        self._n = torch.empty(N, dtype=torch.float32, device=dev)
        self._p = torch.empty((N, d), dtype=torch.float32, device=dev)
        self._scal = torch.empty(8 * N, dtype=torch.float32, device=dev)
        self._off = torch.empty(N, dtype=torch.int64, device=dev)
        self._rows = torch.empty((self.row_cap, d), dtype=torch.float32, device=dev)
        self._pkeys = torch.empty(self.row_cap, dtype=torch.int64, device=dev) if self.c1_sort else None
        self._dWp = torch.empty((N, d * w), dtype=torch.float32, device=dev)
        self._dbp = torch.empty((N, w), dtype=torch.float32, device=dev)
        self._dhp = torch.empty((N, w), dtype=torch.float32, device=dev)
        self._dqp = torch.empty((N, d), dtype=torch.float32, device=dev)
        self._slot = torch.zeros(max(self.n_users, 1), dtype=torch.int64, device=dev)
        self.t = 0
        self._map = self._hs = self._cnt = self._EF = None     # score()'s workspace
        self._proj = None                                      # c1 W[0:d], Q W[d:2d] + b of algorithm 1 (per score())

    # ------------------------------------------------------------------ the ragged buffer
    def positions(self, users):
        """device scalar (int64): the history positions a batch of these users takes — the sum of their train-row
        lengths, twice in pairwise mode (both sides walk the row)"""
        u = users.long().clamp(0, max(self.n_users - 1, 0))
        return self.d_deg[u].sum() * (2 if self.pairwise else 1)

    def max_positions(self, batches_users):
        """host int: the largest positions() of a list of batches (device user tensors) — one gather over their
        concatenation, one sum per batch length, one scalar copy"""
        if not batches_users:
            return 0
        deg = self.d_deg[torch.cat(batches_users).long().clamp(0, max(self.n_users - 1, 0))]
        sizes = [int(u.numel()) for u in batches_users]
        B = max(sizes)
        full = [k for k, n in enumerate(sizes) if n == B]
        tops = []
        if len(full) == len(sizes) or (len(full) == len(sizes) - 1 and sizes[-1] < B):
            n_full = len(full)
            tops.append(deg[:n_full * B].view(n_full, B).sum(1).max())
            if n_full < len(sizes):
                tops.append(deg[n_full * B:].sum())
        else:                                                  # ragged batch lengths: a sum each
            off = 0
            for n in sizes:
                tops.append(deg[off:off + n].sum())
                off += n
        return int(torch.stack(tops).max().item()) * (2 if self.pairwise else 1)

    def reserve(self, positions):
        """make room for batches of up to `positions` history positions"""
        positions = int(positions)
        if positions > self.row_cap:
            self._rows = None
            self.row_cap = positions
            self._rows = torch.empty((self.row_cap, self.d), dtype=torch.float32, device=self.c1.device)
            if self.c1_sort:
                self._pkeys = torch.empty(self.row_cap, dtype=torch.int64, device=self.c1.device)

    def verify(self):
        """raise if any step so far took more history positions than the buffer held (its gradient rows were lost):
        possible only when step() was given a `positions` smaller than the batch's"""
        need = int(self._need[1].item())
        if need > self.row_cap:
            raise RuntimeError("NAIS: a batch took %d history positions, the buffer holds %d: reserve() more or let "
                               "step() size it (positions=None)" % (need, self.row_cap))

    # ------------------------------------------------------------------ training
    def _apply_rows(self, key, flag):
        var, grad, s0, s1 = getattr(self, key), self.G[key], self.s0[key], self.s1[key]
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

    def _apply_dense(self, keys):
        if self.dense is None:
            for k in keys:
                E.adam_dense(getattr(self, k), self.s0[k], self.s1[k], self.G[k], self.adam, clear_grad=False)
        else:
            self.dense.apply([(getattr(self, k), self.s0[k], self.s1[k], self.G[k], False) for k in keys])

    def step(self, users, items, third, loss_out, positions=None):
        """pointwise: third = labels (float32); pairwise: third = negative items (int32).  loss_out: 2 floats on the
        device, (loss term, regulariser term) of the batch before the update.  positions: an upper bound of
        self.positions(users) the caller already has on the host (the plugin takes one per epoch); None: the engine
        reads it from the device, one scalar copy per step.  A `positions` smaller than the batch's is found LATE: the
        kernels write nothing beyond the buffer, the step is applied without the lost gradient rows, and the next
        verify() raises — a caller that passes a figure calls verify() before it trusts the tables."""
        B = int(users.numel())
        self.reserve(int(self.positions(users).item()) if positions is None else positions)
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if items.numel() != B or third.numel() != B:
            raise ValueError("users, items and the third field must have the same length")
        self.t += 1
        a = NaisStepArgs()
        a.indptr, a.indices = _ptr(self.csr.indptr, torch.int64), _ptr(self.csr.indices, torch.int32)
        a.t_indptr, a.t_users = _ptr(self.csc.indptr, torch.int64), _ptr(self.csc.indices, torch.int32)
        a.c1, a.Q, a.bias, a.W, a.b, a.h = (_ptr(getattr(self, k)) for k in self._names)
        a.G_c1, a.G_Q, a.G_bias, a.G_W, a.G_b, a.G_h = (_ptr(self.G[k]) for k in self._names)
        a.flag_Q, a.flag_bias, a.flag_c1 = _addr(self.flag_Q), _addr(self.flag_bias), _addr(self.flag_c1)
        a.users, a.items = _ptr(users, torch.int32), _ptr(items, torch.int32)
        a.third = _ptr(third, torch.int32 if self.pairwise else torch.float32)
        a.keys, a.inst, a.n, a.p, a.scal = (_ptr(t) for t in (self._keys, self._inst, self._n, self._p, self._scal))
        a.slot, a.off, a.rows = _ptr(self._slot), _ptr(self._off), _ptr(self._rows)
        a.need = _ptr(self._need, torch.int64)
        a.pkeys, a.c1_sort = _addr(self._pkeys), int(self.c1_sort)
        a.dWp, a.dbp, a.dhp, a.dqp = _ptr(self._dWp), _ptr(self._dbp), _ptr(self._dhp), _ptr(self._dqp)
        a.loss2 = _ptr(loss_out, torch.float32)
        a.row_cap = self.row_cap
        a.n_users, a.n_items, a.d, a.w, a.batch = self.n_users, self.n_items, self.d, self.w, B
        a.pairwise, a.loss_kind, a.step = int(self.pairwise), self.loss_kind, self.t
        a.algorithm, a.activation, a.reference_mask = self.algorithm, self.activation, int(self.reference_mask)
        a.alpha, a.beta, a.reg_p, a.reg_q = self.alpha, self.beta, self.reg_p, self.reg_q
        call("nrhip_nais_step", C.byref(a), _stream())
        if self.c1_rows:
            self._apply_rows("c1", self.flag_c1)
            self._apply_dense(("W", "b", "h"))
        else:
            self._apply_dense(("c1", "W", "b", "h"))
        self._apply_rows("Q", self.flag_Q)
        self._apply_rows("bias", self.flag_bias)
        self.adam.advance()

    # ------------------------------------------------------------------ scoring
    def score(self, users):
        """S [B, I] float32 on the device: NAIS.py:246-257 for `users`, every item, own items included"""
        dev = self.c1.device
        if isinstance(users, torch.Tensor):
            h_users = users.detach().cpu().numpy().astype(np.int64)
        else:
            h_users = np.asarray(users, dtype=np.int64)
        users = torch.from_numpy(np.ascontiguousarray(h_users, dtype=np.int32)).to(dev)
        B, I = int(users.numel()), self.n_items
        out = torch.empty((B, I), dtype=torch.float32, device=dev)
        if B == 0 or I == 0:
            return out
        ok = (h_users >= 0) & (h_users < self.n_users)
        h_cap = int(min(I, max(1, int(self.h_deg[h_users[ok]].sum()))))
        tile = (SCORE_WS_BYTES // (8 * h_cap)) // 256 * 256
        tile = int(min(max(tile, 256), (I + 255) // 256 * 256))
        if self._map is None:
            self._map = torch.empty(I, dtype=torch.int32, device=dev)
            self._hs = torch.empty(I, dtype=torch.int32, device=dev)
            self._cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        if self._EF is None or self._EF.numel() < 2 * h_cap * tile:
            self._EF = None
            self._EF = torch.empty(2 * h_cap * tile, dtype=torch.float32, device=dev)
        project = 0
        if self.algorithm == 1:
            # made again by every call (I d w multiply-adds, nothing beside the pairs): a table assigned between two
            # calls can never be scored with projections of the one before
            if self._proj is None:
                self._proj = (None, torch.empty((I, self.w), dtype=torch.float32, device=dev),
                              torch.empty((I, self.w), dtype=torch.float32, device=dev))
            project = 1
        for s in range(0, B, 65535):
            blk = users[s:s + 65535]
            a = NaisScoresArgs()
            a.indptr, a.indices = _ptr(self.csr.indptr, torch.int64), _ptr(self.csr.indices, torch.int32)
            a.c1, a.Q, a.bias, a.W, a.b, a.h = (_ptr(getattr(self, k)) for k in self._names)
            a.users, a.out = _ptr(blk, torch.int32), C.c_void_p(out[s:].data_ptr())
            a.map, a.hs, a.cnt = _ptr(self._map), _ptr(self._hs), _ptr(self._cnt)
            a.E, a.F = C.c_void_p(self._EF.data_ptr()), C.c_void_p(self._EF.data_ptr() + 4 * h_cap * tile)
            if self.algorithm == 1:
                a.cW, a.qW = _ptr(self._proj[1]), _ptr(self._proj[2])
            a.ld = out.stride(0)
            a.n_users, a.n_items, a.d, a.w = self.n_users, I, self.d, self.w
            a.algorithm, a.activation, a.batch = self.algorithm, self.activation, int(blk.numel())
            a.h_cap, a.tile, a.project, a.mfma = h_cap, tile, project, int(self.mfma)
            a.alpha, a.beta = self.alpha, self.beta
            call("nrhip_nais_scores", C.byref(a), _stream())
            project = 0
        return out
