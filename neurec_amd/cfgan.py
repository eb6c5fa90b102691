"""CFGAN on the HIP engine: the masks of CFGAN.py:135-148, one `sess.run(trainer_d)` / `sess.run(trainer_g)` per step
(CFGAN.py:60-95) and the ratings of CFGAN.py:183-193 (csrc/cfgan.hip).

R is the train matrix in CSR, transposed for itemBased; a batch is a list of its rows.  The generator G maps a row c to
`out` [B, n_cols]; the discriminator D sees [c | c] and [c | out . pm].  Per outer epoch every row with a train entry
gets two masks, zr and pm: its positives plus int((n_cols - deg) ratio) other columns.  Here a mask is a bit row that the
device builds from (seed, epoch, plane, row id) when the row's batch comes up, so only [B, n_cols] bits exist at a time;
`masks_given` takes bit rows laid out by the host instead (the reference's recorded draws).

Two optimisers with disjoint variable lists take turns: `d_step` moves D's kernels and biases and reads G, `g_step`
moves G's and reads D.  Each is its own Adam (own beta powers, advanced on its own steps only) or gradient descent; every
variable is consumed by a matmul, so every update is the dense form.  The regularisers reg . sum(v^2) / 2 over a
network's kernels AND biases ride on the optimiser pass: its gradient is g + reg v, its loss term the sum it reads.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import torch

from . import engine as E
from ._lib import CfganNet, CfganStepArgs, call
from .engine import _ptr, _stream
from .row_learner import f32

MAX_HIDDEN = 3                # NRHIP_CFGAN_MAX_HIDDEN
MAX_WIDTH = 512               # NRHIP_CFGAN_MAX_WIDTH
MAX_BATCH = 1024              # NRHIP_CFGAN_MAX_BATCH
APPLY_BLOCKS = 2048           # NRHIP_CFGAN_APPLY_BLOCKS
MAX_COLS = (1 << 24) - 1
MODES = ("userBased", "itemBased")
OPTS = ("adam", "sgd")
_MASK64 = (1 << 64) - 1


def table_names(n_g, n_d):
    """the variables in the reference's creation order: gen_h*, gen_out, dis_h*, dis_out, kernel before bias"""
    out = []
    for net, n in (("gen", n_g), ("dis", n_d)):
        for k in range(n):
            out += ["%s_h%d_kernel" % (net, k), "%s_h%d_bias" % (net, k)]
        out += ["%s_out_kernel" % net, "%s_out_bias" % net]
    return out


def check_config(mode, hidden_g, hidden_d, batch_g, batch_d, opt_g, opt_d, zr_ratio, zp_ratio):
    """the refusals of this engine, each naming its key and the supported range"""
    if mode not in MODES:
        raise ValueError("CFGAN: mode=%r is not supported (userBased or itemBased)" % (mode,))
    for key, opt in (("opt_G", opt_g), ("opt_D", opt_d)):
        if opt not in OPTS:
            raise ValueError("CFGAN: %s=%r is not supported (adam or sgd)" % (key, opt))
    for key, widths in (("hiddenLayer_G", hidden_g), ("hiddenLayer_D", hidden_d)):
        widths = list(widths)
        if not 1 <= len(widths) <= MAX_HIDDEN:
            raise NotImplementedError("CFGAN: %s=%r is not supported (1 to %d hidden layers)" % (key, widths, MAX_HIDDEN))
        if any(int(w) < 1 or int(w) > MAX_WIDTH for w in widths):
            raise NotImplementedError("CFGAN: %s=%r is not supported (widths 1 to %d)" % (key, widths, MAX_WIDTH))
    for key, b in (("batchSize_G", batch_g), ("batchSize_D", batch_d)):
        if int(b) < 1 or int(b) > MAX_BATCH:
            raise NotImplementedError("CFGAN: %s=%d is not supported (1 to %d rows)" % (key, int(b), MAX_BATCH))
    for key, r in (("ZR_ratio", zr_ratio), ("ZP_ratio", zp_ratio)):
        if not 0.0 <= float(r) <= 1.0:
            raise ValueError("CFGAN: %s=%r is not supported (0 to 1)" % (key, r))


def _host_ids(x):
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32)


class CFGANMasks:
    """the two bit planes of one batch on the device: zr, pm uint32-as-int32 [B, words]; host(): numpy uint32 copies"""

    def __init__(self, rows, zr, pm, n_cols):
        self.rows, self.zr, self.pm, self.n_cols = rows, zr, pm, int(n_cols)

    def host(self):
        return tuple(t.cpu().numpy().view(np.uint32) for t in (self.zr, self.pm))

    def dense(self):
        """(zr, pm) as bool [B, n_cols] on the host"""
        out = []
        for bits in self.host():
            flat = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8).reshape(len(bits), -1), axis=1,
                                 bitorder="little")
            out.append(flat[:, :self.n_cols].astype(bool))
        return tuple(out)


class _Net:
    """one network's variables, gradients and optimiser state, and its nrhip_cfgan_net"""

    def __init__(self, net, tables, widths, n_in, n_out, opt, lr, dev):
        self.net, self.widths, self.n_in, self.n_out, self.opt = net, [int(w) for w in widths], int(n_in), int(n_out), opt
        self.names = [("%s_h%d_kernel" % (net, k), "%s_h%d_bias" % (net, k)) for k in range(len(widths))] + \
            [("%s_out_kernel" % net, "%s_out_bias" % net)]
        self.T, dims = {}, [self.n_in] + self.widths + [self.n_out]
        for k, (kn, bn) in enumerate(self.names):
            W, b = f32(tables[kn]), f32(tables[bn])
            if tuple(W.shape) != (dims[k], dims[k + 1]) or tuple(b.shape) != (dims[k + 1],):
                raise ValueError("CFGAN: %s must be [%d, %d] and %s [%d]" % (kn, dims[k], dims[k + 1], bn, dims[k + 1]))
            self.T[kn], self.T[bn] = W.contiguous().to(dev), b.contiguous().to(dev)
        self.G = {k: torch.zeros_like(t) for k, t in self.T.items()}
        adam = opt == "adam"
        self.m = {k: torch.zeros_like(t) for k, t in self.T.items()} if adam else {}
        self.v = {k: torch.zeros_like(t) for k, t in self.T.items()} if adam else {}
        self.adam = E.AdamState(lr)                            # its own beta powers; t counts this network's steps
        self.lr = float(lr)
        self.c = CfganNet()
        self.c.n_hidden = len(self.widths)
        for k, w in enumerate(self.widths):
            self.c.width[k] = w
        for k, (kn, bn) in enumerate(self.names):
            self.c.W[k], self.c.b[k] = self.T[kn].data_ptr(), self.T[bn].data_ptr()
            self.c.G_W[k], self.c.G_b[k] = self.G[kn].data_ptr(), self.G[bn].data_ptr()
            if adam:
                self.c.m_W[k], self.c.m_b[k] = self.m[kn].data_ptr(), self.m[bn].data_ptr()
                self.c.v_W[k], self.c.v_b[k] = self.v[kn].data_ptr(), self.v[bn].data_ptr()

    def apply(self, reg, partials, loss_slot):
        """gradient + reg v, the optimiser, the gradient cleared; loss_slot = reg sum(v^2) / 2 before the update"""
        st = self.adam
        call("nrhip_cfgan_apply", C.byref(self.c), self.n_in, self.n_out, 0 if self.opt == "adam" else 1,
             float(st.alpha()) if self.opt == "adam" else self.lr, float(st.beta1), float(st.beta2), float(st.eps),
             float(reg), _ptr(partials, torch.float64), C.c_void_p(loss_slot.data_ptr()), _stream())
        st.advance()


class CFGANEngine:
    """Both networks, their optimiser states and gradient buffers in HBM, and the CSR of R.

    `train`: [num_users, num_items]; itemBased transposes it here.  rows are host ids of R's rows, repeats allowed.
    `d_step(rows, loss_out)` / `g_step(rows, loss_out)`: one step; loss_out holds 3 device floats — D writes (real, fake,
    regulariser), G (adversarial, regulariser, zero-reconstruction), all from before the update.  `masks=None` builds the
    batch's masks on the device from (seed, self.epoch); `score(users)` -> [B, num_items] on the device."""

    def __init__(self, tables, train, hidden_g, hidden_d, lr_G, lr_D, reg_G, reg_D, zr_ratio, zp_ratio, zr_coef,
                 batch_g, batch_d, opt_G="adam", opt_D="adam", mode="userBased", seed=2018):
        check_config(mode, hidden_g, hidden_d, batch_g, batch_d, opt_G, opt_D, zr_ratio, zp_ratio)
        M = sp.csr_matrix(train)
        self.num_users, self.num_items = M.shape
        if mode == "itemBased":
            M = M.transpose().tocsr()
        M.sum_duplicates()
        M.sort_indices()
        self.n_rows, self.n_cols = M.shape
        if not 1 <= self.n_cols <= MAX_COLS:
            raise NotImplementedError("CFGAN: %d columns are not supported (1 to %d)" % (self.n_cols, MAX_COLS))
        dev = E.require_gpu()
        self.dev, self.mode, self.seed, self.epoch = dev, mode, int(seed) & _MASK64, 0
        self.csr = E.DeviceCSR.from_scipy(M)
        self.h_indptr = np.asarray(M.indptr, dtype=np.int64)
        self.h_deg = np.diff(self.h_indptr)
        self.zr_ratio, self.zp_ratio, self.zr_coef = float(zr_ratio), float(zp_ratio), float(zr_coef)
        self.reg_G, self.reg_D = float(reg_G), float(reg_D)
        self.batch_g, self.batch_d = int(batch_g), int(batch_d)
        self.max_batch = max(self.batch_g, self.batch_d)
        self.words = (self.n_cols + 31) // 32
        self.gen = _Net("gen", tables, hidden_g, self.n_cols, self.n_cols, opt_G, lr_G, dev)
        self.dis = _Net("dis", tables, hidden_d, 2 * self.n_cols, 1, opt_D, lr_D, dev)
        # the sample sizes as the reference computes them, in Python doubles; a row without a train entry has no masks
        self.h_counts = np.asarray([[int((self.n_cols - int(d)) * self.zr_ratio) if d else 0,
                                     int((self.n_cols - int(d)) * self.zp_ratio) if d else 0] for d in self.h_deg],
                                   dtype=np.int32).reshape(-1, 2)
        a = self._args()
        floats, nbytes = C.c_size_t(0), C.c_size_t(0)
        call("nrhip_cfgan_workspace", C.byref(a), C.byref(floats), C.byref(nbytes))
        self._ws = torch.empty(max(floats.value, 1), dtype=torch.float32, device=dev)
        self._gemm_ws = torch.empty(max(nbytes.value, 256), dtype=torch.uint8, device=dev)
        self._partials = torch.zeros(APPLY_BLOCKS, dtype=torch.float64, device=dev)
        self._keys = None
        self._version = 0                                      # bumped by every g_step: the scorer's tables are G's
        self._gemm = None                                      # [the scoring GEMM, the version its items were prepared at]
        self._items = None

    # ------------------------------------------------------------------ plumbing
    @property
    def T(self):
        """{name: device tensor} of every variable"""
        return {**self.gen.T, **self.dis.T}

    @property
    def G(self):
        return {**self.gen.G, **self.dis.G}

    def _args(self):
        a = CfganStepArgs()
        a.gen, a.dis = self.gen.c, self.dis.c
        a.indptr, a.indices = _ptr(self.csr.indptr, torch.int64), _ptr(self.csr.indices, torch.int32)
        a.n_rows, a.n_cols, a.max_batch, a.zr_coef = self.n_rows, self.n_cols, self.max_batch, self.zr_coef
        return a

    def _rows(self, rows):
        h = _host_ids(rows)
        if len(h) > self.max_batch:
            raise ValueError("CFGAN: a batch of %d rows, the engine was made for %d" % (len(h), self.max_batch))
        if len(h) and (h.min() < 0 or h.max() >= self.n_rows):
            raise ValueError("CFGAN: row ids must lie in [0, %d)" % self.n_rows)
        return h

    # ------------------------------------------------------------------ masks
    def masks(self, rows, epoch=None):
        """the masks of `rows` at outer epoch `epoch` (None: self.epoch), built on the device"""
        h = self._rows(rows)
        return self.masks_counts(h, self.h_counts[h], self.epoch if epoch is None else epoch)

    def masks_counts(self, rows, counts, epoch):
        """as masks(), with the sample sizes [B, 2] given instead of computed from the ratios (tests)"""
        h = self._rows(rows)
        B, dev = len(h), self.dev
        counts = np.ascontiguousarray(np.asarray(counts, dtype=np.int32).reshape(B, 2))
        zr, pm = (torch.zeros((B, self.words), dtype=torch.int32, device=dev) for _ in range(2))
        if B:
            rows_d, counts_d = torch.from_numpy(h).to(dev), torch.from_numpy(counts).to(dev)
            call("nrhip_cfgan_masks", _ptr(self.csr.indptr), _ptr(self.csr.indices), _ptr(rows_d), _ptr(counts_d), B,
                 self.n_rows, self.n_cols, self.seed, int(epoch) & _MASK64, _ptr(zr), _ptr(pm), _stream())
        return CFGANMasks(h, zr, pm, self.n_cols)

    def masks_given(self, rows, zr_bits, pm_bits):
        """masks laid out by the host: uint32 [B, ceil(n_cols / 32)] each, column 32 w + k at bit k of word w"""
        h = self._rows(rows)
        planes = []
        for bits in (zr_bits, pm_bits):
            bits = np.ascontiguousarray(np.asarray(bits, dtype=np.uint32).reshape(len(h), -1))
            if bits.shape[1] != self.words:
                raise ValueError("CFGAN: a mask row holds %d words, %d expected" % (bits.shape[1], self.words))
            if self.n_cols % 32 and len(h) and (bits[:, -1] >> np.uint32(self.n_cols % 32)).any():
                raise ValueError("CFGAN: mask bits beyond column %d" % self.n_cols)
            planes.append(torch.from_numpy(bits.view(np.int32)).to(self.dev))
        return CFGANMasks(h, planes[0], planes[1], self.n_cols)

    # ------------------------------------------------------------------ the steps
    def _gradients(self, which, rows, loss_out, masks):
        h = self._rows(rows)
        B = len(h)
        if masks is None:
            masks = self.masks(h)
        elif not np.array_equal(masks.rows, h):
            raise ValueError("CFGAN: the masks were made for other rows")
        ent_ptr = np.concatenate([[0], np.cumsum(self.h_deg[h])]).astype(np.int64)
        n_ent = int(ent_ptr[-1])
        if self._keys is None or self._keys.numel() < n_ent:
            self._keys = torch.empty(max(n_ent, 1), dtype=torch.int64, device=self.dev)
        rows_d, ent_d = torch.from_numpy(h).to(self.dev), torch.from_numpy(ent_ptr).to(self.dev)
        a = self._args()
        a.rows, a.ent_ptr, a.zr, a.pm = _ptr(rows_d), _ptr(ent_d), _ptr(masks.zr), _ptr(masks.pm)
        a.keys, a.ws, a.gemm_ws, a.gemm_ws_bytes = _ptr(self._keys), _ptr(self._ws), _ptr(self._gemm_ws), \
            self._gemm_ws.numel()
        a.loss3 = _ptr(loss_out, torch.float32)
        a.batch, a.n_ent = B, n_ent
        call("nrhip_cfgan_d_step" if which == "d" else "nrhip_cfgan_g_step", C.byref(a), _stream())

    def d_step(self, rows, loss_out, masks=None):
        """one trainer_d run on `rows`: moves D's kernels and biases only.  An empty batch is a no-op."""
        if len(rows) == 0:
            return
        self._gradients("d", rows, loss_out, masks)
        self.dis.apply(self.reg_D, self._partials, loss_out[2:3])

    def g_step(self, rows, loss_out, masks=None):
        """one trainer_g run on `rows`: moves G's kernels and biases only.  An empty batch is a no-op."""
        if len(rows) == 0:
            return
        self._gradients("g", rows, loss_out, masks)
        self.gen.apply(self.reg_G, self._partials, loss_out[1:2])
        self._version += 1

    # ------------------------------------------------------------------ scoring
    def hidden(self, rows):
        """[B, w + 1] rows [G's last hidden layer of R's row | 1]; rows None: every row of R"""
        h = None if rows is None else _host_ids(rows)
        B, w = self.n_rows if h is None else len(h), self.gen.widths[-1]
        if h is not None and B and (h.min() < 0 or h.max() >= self.n_rows):
            raise ValueError("CFGAN: row ids must lie in [0, %d)" % self.n_rows)
        out = torch.empty((B, w + 1), dtype=torch.float32, device=self.dev)
        if B == 0:
            return out
        out[:, w] = 1.0
        tmp = torch.empty(2 * B * MAX_WIDTH, dtype=torch.float32, device=self.dev) if len(self.gen.widths) > 1 else None
        rows_d = None if h is None else torch.from_numpy(h).to(self.dev)
        call("nrhip_cfgan_hidden", C.byref(self.gen.c), _ptr(self.csr.indptr), _ptr(self.csr.indices),
             _ptr(rows_d, allow_none=True), B, self.n_cols, _ptr(tmp, allow_none=True), _ptr(out), out.stride(0),
             _stream())
        return out

    def _out_table(self):
        """[n_cols, w + 1] rows [Wg2[:, i] | bg2[i]]"""
        return torch.cat([self.gen.T["gen_out_kernel"].t(), self.gen.T["gen_out_bias"].reshape(-1, 1)], dim=1).contiguous()

    def factors(self, users):
        """(user factors [B, w + 1], item factors [num_items, w + 1]); the item side is made once per state of G"""
        users = _host_ids(users)
        if len(users) and (users.min() < 0 or users.max() >= self.num_users):
            raise ValueError("CFGAN: user ids must lie in [0, %d)" % self.num_users)
        if self._items is None or self._items[0] != self._version:
            self._items = (self._version, self._out_table() if self.mode == "userBased" else self.hidden(None))
        if self.mode == "userBased":
            return self.hidden(users), self._items[1]
        idx = torch.from_numpy(users.astype(np.int64)).to(self.dev)
        F = torch.cat([self.gen.T["gen_out_kernel"][:, idx].t(), self.gen.T["gen_out_bias"][idx].reshape(-1, 1)], dim=1)
        return F.contiguous(), self._items[1]

    def score(self, users):
        """S [B, num_items] float32 on the device: all_ratings[users] of CFGAN.py:183-190"""
        F, items = self.factors(users)
        B = int(F.shape[0])
        if B == 0:
            return torch.empty((0, self.num_items), dtype=torch.float32, device=self.dev)
        if self._gemm is None or self._gemm[0].max_rows < B:
            self._gemm = [E.score_gemm_for(items, max(B, 1)), self._version]
        elif self._gemm[1] != self._version:
            self._gemm[0].prepare(items)
            self._gemm[1] = self._version
        return self._gemm[0](F, None)[:, :self.num_items]

    def forward(self, users, items, sizes=None):
        """candidate mode: the scores of the flat `items`, sizes[b] of them for users[b] (None: one each)"""
        F, Q = self.factors(users)
        it = _host_ids(items)
        sizes = np.ones(F.shape[0], np.int64) if sizes is None else np.asarray(sizes, dtype=np.int64)
        if int(sizes.sum()) != len(it) or len(sizes) != F.shape[0]:
            raise ValueError("sizes must hold one count per user and sum to the number of items")
        if len(it) and (it.min() < 0 or it.max() >= self.num_items):
            raise ValueError("CFGAN: item ids must lie in [0, %d)" % self.num_items)
        out = torch.empty(len(it), dtype=torch.float32, device=self.dev)
        if len(it) == 0:
            return out
        rows = torch.from_numpy(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)).to(self.dev)
        items_d = torch.from_numpy(it).to(self.dev)
        call("nrhip_cfgan_pairs", _ptr(F), F.stride(0), _ptr(Q), Q.stride(0), int(F.shape[1]), _ptr(rows),
             _ptr(items_d), len(it), _ptr(out), _stream())
        return out

    def tables(self):
        """{name: numpy copy} of every variable, in creation order"""
        T = self.T
        return {k: T[k].cpu().numpy() for k in table_names(len(self.gen.widths), len(self.dis.widths))}
