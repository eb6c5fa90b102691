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
import torch

from ._lib import NaisScoresArgs, NaisStepArgs, call
from .engine import _ptr, _stream
from .history import HistoryEngine
from .row_learner import addr, f32

MAX_D = 128                   # NRHIP_NAIS_MAX_D
MAX_W = 64                    # NRHIP_NAIS_MAX_W
ACTIVATIONS = {0: "relu", 1: "sigmoid", 2: "tanh"}
SCORE_WS_BYTES = 256 << 20    # the two [history items, tile] buffers of score()


C1_PATH = "walk"              # how G_c1 is summed: "walk" or "sort" (DESIGN 6e has the A/B)
PAIR_KERNEL = "mfma"          # score()'s pair kernel where both exist (algorithm 0, d <= 16, w <= 16): "valu" or "mfma"


def activation_code(activation):
    """NAIS.py:158-163 compares conf["activation"] with the ints 0 / 1 / 2; anything else applies no activation"""
    for k in ACTIVATIONS:
        if type(activation) in (int, np.int32, np.int64) and activation == k:
            return k
    return 3


class NAISEngine(HistoryEngine):
    """Tables c1 / Q / bias / W / b / h, their optimiser state and gradient buffers in HBM (neurec_amd/history.py).

    `step(users, items, third, loss_out)`: one batch of the device instance stream, as FISMEngine.step.
    `score(users)` -> [B, I] on the device: predict() on the whole train row."""
    NAME, MAX_D, ARGS, STEP = "NAIS", MAX_D, NaisStepArgs, "nrhip_nais_step"

    def __init__(self, c1, Q, W, b, train, lr, regs, alpha, beta, max_batch, algorithm=0, activation=None,
                 loss="cross_entropy", pairwise=False, learner="adam", bias=None, h=None, momentum=0.9,
                 attention_mask="reference", c1_application="dense", c1_path=C1_PATH, pair_kernel="auto",
                 more_dense=None, q_application="rows"):
        """more_dense(d): further dense variables of a model that pools as NAIS does (neurec_amd/deepicf.py);
        q_application: HistoryEngine's"""
        if attention_mask not in ("reference", "history"):
            raise ValueError("attention_mask is 'reference' or 'history', got %r" % (attention_mask,))
        if algorithm not in (0, 1):
            raise ValueError("algorithm is 0 (product) or 1 (concat), got %r" % (algorithm,))
        if not float(beta) >= 0.0:
            raise ValueError("NAIS needs beta >= 0, got %r" % (beta,))
        if c1_path not in ("walk", "sort"):
            raise ValueError("c1_path is 'walk' or 'sort', got %r" % (c1_path,))
        if pair_kernel not in ("auto", "valu", "mfma"):
            raise ValueError("pair_kernel is 'auto', 'valu' or 'mfma', got %r" % (pair_kernel,))

        def attention(d):
            Wt, bt = f32(W), f32(b).reshape(-1)
            if Wt.dim() != 2 or Wt.shape[0] != (algorithm + 1) * d:
                raise ValueError("W must be [%d, weight_size]" % ((algorithm + 1) * d,))
            w = int(Wt.shape[1])
            if w < 1 or w > MAX_W:
                raise NotImplementedError("NAIS: weight_size=%d is not supported (1 to %d)" % (w, MAX_W))
            ht = torch.ones(w) if h is None else f32(h).reshape(-1)
            if bt.numel() != w or ht.numel() != w:
                raise ValueError("b and h must hold weight_size entries")
            return dict({"W": Wt, "b": bt, "h": ht}, **(more_dense(d) if more_dense else {}))
        # sorted rows: the walk finds an item in a row by bisection.  regs[2] is read and never used (NAIS.py:33)
        HistoryEngine.__init__(self, c1, Q, train, lr, regs, alpha, max_batch, loss, pairwise, learner, bias, momentum,
                               c1_application, dense=attention, sorted_rows=True, q_application=q_application)
        dev, d, N = self.c1.device, self.d, self._N
        w = self.w = int(self.W.shape[1])
        mfma_ok = algorithm == 0 and d <= 16 and w <= 16
        if pair_kernel == "mfma" and not mfma_ok:
            raise NotImplementedError("NAIS: the matrix-core pair kernel takes algorithm 0 with embedding_size <= 16 "
                                      "and weight_size <= 16")
        self.algorithm, self.activation, self.beta = int(algorithm), activation_code(activation), float(beta)
        self.reference_mask = attention_mask == "reference"
        self.c1_sort = c1_path == "sort"
        self.mfma = (PAIR_KERNEL if pair_kernel == "auto" else pair_kernel) == "mfma" and mfma_ok
        # the ragged [positions, d] buffer holds one row per history position of the BATCH (an instance takes its
        # user's train-row length); it starts at the mean batch's size and grows to what a batch asks (reserve)
        self.d_deg = torch.from_numpy(self.h_deg).to(dev)
        self._need = torch.zeros(2, dtype=torch.int64, device=dev)
        self.row_cap = max(64, int(np.ceil(N * float(self.h_deg.mean() if len(self.h_deg) else 0.0))))
        self._off = torch.empty(N, dtype=torch.int64, device=dev)
        self._rows = torch.empty((self.row_cap, d), dtype=torch.float32, device=dev)
        self._pkeys = torch.empty(self.row_cap, dtype=torch.int64, device=dev) if self.c1_sort else None
        self._dWp = torch.empty((N, d * w), dtype=torch.float32, device=dev)
        self._dbp = torch.empty((N, w), dtype=torch.float32, device=dev)
        self._dhp = torch.empty((N, w), dtype=torch.float32, device=dev)
        self._dqp = torch.empty((N, d), dtype=torch.float32, device=dev)
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
    def _fill(self, a):
        a.off, a.rows, a.need = _ptr(self._off), _ptr(self._rows), _ptr(self._need, torch.int64)
        a.pkeys, a.c1_sort = addr(self._pkeys), int(self.c1_sort)
        a.dWp, a.dbp, a.dhp, a.dqp = _ptr(self._dWp), _ptr(self._dbp), _ptr(self._dhp), _ptr(self._dqp)
        a.row_cap, a.w, a.beta = self.row_cap, self.w, self.beta
        a.algorithm, a.activation, a.reference_mask = self.algorithm, self.activation, int(self.reference_mask)

    def step(self, users, items, third, loss_out, positions=None):
        """as HistoryEngine.step.  positions: an upper bound of self.positions(users) the caller already has on the
        host (the plugin takes one per epoch); None: the engine reads it from the device, one scalar copy per step.  A
        `positions` smaller than the batch's is found LATE: the kernels write nothing beyond the buffer, the step is
        applied without the lost gradient rows, and the next verify() raises — a caller that passes a figure calls
        verify() before it trusts the tables."""
        self.reserve(int(self.positions(users).item()) if positions is None else positions)
        HistoryEngine.step(self, users, items, third, loss_out)

    # ------------------------------------------------------------------ scoring
    def _scores_call(self, a):
        call("nrhip_nais_scores", C.byref(a), _stream())

    def score(self, users, call=None):
        """S [B, I] float32 on the device: NAIS.py:246-257 for `users`, every item, own items included.  call(a): what
        runs per block of users on the filled argument struct (None: nrhip_nais_scores)"""
        call = call or self._scores_call
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
            a.c1, a.Q, a.bias, a.W, a.b, a.h = (_ptr(getattr(self, k)) for k in self._names[:6])
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
            call(a)
            project = 0
        return out
