"""IRGAN on the HIP engine: the discriminator's training data (IRGAN.py:162-193), one `sess.run(d_updates)` per batch
(IRGAN.py:102-107, 203-211), the generator's user steps (IRGAN.py:213-235) and the ratings (csrc/irgan.hip).

Two triples (P [U, d], Q [I, d], b [I]): G, the generator, and D, the discriminator; plain gradient descent with one lr,
no optimiser slots.  A D pass draws deg(u) items per train user from softmax((P_g[u] Q_g^T + b_g) / d_tau) — blocks of
users through the scoring GEMM on [P | 1], [Q | b], integer weights in place of the slab, draws on the device — and runs
its batches without returning to Python.  A G pass is one user step after the other: the next user's logits depend on
this user's dense update of Q_g and b_g.  A draw is a pure function of (seed, pass counter, phase, user, draw index); the
pass counters advance once per `d_data()` and once per `g_pass()`.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import torch

from . import engine as E
from ._lib import IrganArgs, call
from .engine import _ptr, _stream
from .row_learner import f32

MAX_D = 128                    # NRHIP_IRGAN_MAX_D
MAX_BATCH = 1024               # NRHIP_IRGAN_MAX_BATCH
SLAB_FLOATS = 1 << 28          # a D-data block's score slab stays below this
NAMES = ("g_P", "g_Q", "g_b", "d_P", "d_Q", "d_b")
_MASK64 = (1 << 64) - 1


def check_config(factors_num, batch_size, d_tau, g_reg, d_reg, lr):
    """the refusals of this engine, each naming its key and the supported range"""
    if not 1 <= int(factors_num) <= MAX_D:
        raise NotImplementedError("IRGAN: factors_num=%d is not supported (1 to %d)" % (int(factors_num), MAX_D))
    if not 1 <= int(batch_size) <= MAX_BATCH:
        raise NotImplementedError("IRGAN: batch_size=%d is not supported (1 to %d)" % (int(batch_size), MAX_BATCH))
    if not float(d_tau) > 0.0:
        raise ValueError("IRGAN: d_tau=%r is not supported (above 0)" % (d_tau,))
    for key, reg in (("g_reg", g_reg), ("d_reg", d_reg)):
        if not float(reg) >= 0.0:
            raise ValueError("IRGAN: %s=%r is not supported (0 or more)" % (key, reg))
    if not float(lr) > 0.0:
        raise ValueError("IRGAN: lr=%r is not supported (above 0)" % (lr,))


def train_users_of(indptr, indices):
    """IRGAN.py:142-147: the rows for which `any(row.indices)` is true — a user without a train item is left out, and so
    is one whose only train item is item 0"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices)
    nz = np.concatenate([[0], np.cumsum(indices != 0)])
    return np.nonzero(nz[indptr[1:]] - nz[indptr[:-1]] > 0)[0].astype(np.int32)


def _ids(x):
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32)


class IRGANEngine:
    """Both triples in HBM, the train CSR, the train users under the reference's any() rule, the pass counters.

    `tables`: {g_P, g_Q, g_b, d_P, d_Q, d_b}.  `d_data()` -> (users, items, labels) on the device, interleaved
    (u, pos_k, 1), (u, draw_k, 0) per train user in ascending id; `d_pass(order)` draws them and steps through the batches
    of the shuffled index array; `d_step(users, items, labels, loss_out)` is one step on given triples; `g_step(user,
    samples)` one user step (recorded samples in place of made ones), `g_pass()` all train users.  After a G step
    `last_weights()` and `last_draws()` read what it drew from and what it drew."""

    def __init__(self, tables, train, lr, g_reg, d_reg, d_tau, batch_size, seed=2018):
        M = sp.csr_matrix(train)
        M.sum_duplicates()
        M.sort_indices()
        self.num_users, self.num_items = M.shape
        for k in NAMES:
            if k not in tables:
                raise ValueError("IRGAN: the table %s is missing" % k)
        d = int(np.asarray(tables["g_P"]).shape[1]) if np.asarray(tables["g_P"]).ndim == 2 else 0
        check_config(d, batch_size, d_tau, g_reg, d_reg, lr)
        if self.num_items < 1:
            raise ValueError("IRGAN: the train matrix has no item")
        dev = E.require_gpu()
        self.dev, self.d, self.seed = dev, d, int(seed) & _MASK64
        shapes = {"P": (self.num_users, d), "Q": (self.num_items, d), "b": (self.num_items,)}
        self.T = {}
        for k in NAMES:
            t = f32(tables[k])
            if tuple(t.shape) != shapes[k[2]]:
                raise ValueError("IRGAN: %s must be %s, got %s" % (k, list(shapes[k[2]]), list(t.shape)))
            self.T[k] = t.contiguous().to(dev).clone()
        self.lr, self.g_reg, self.d_reg, self.d_tau = float(lr), float(g_reg), float(d_reg), float(d_tau)
        self.batch_size = int(batch_size)
        self.csr = E.DeviceCSR.from_scipy(M)
        self.h_indptr = np.asarray(M.indptr, np.int64)
        self.h_indices = np.asarray(M.indices, np.int32)
        self.h_deg = np.diff(self.h_indptr)
        self.train_users = train_users_of(self.h_indptr, self.h_indices)
        self.max_deg = max(int(self.h_deg.max(initial=0)), 1)
        self.d_passes = self.g_passes = 0
        floats = C.c_size_t(0)
        call("nrhip_irgan_workspace", self.num_items, d, MAX_BATCH, C.byref(floats))
        self._ws = torch.empty(max(floats.value, 1), dtype=torch.float32, device=dev)
        self._z = torch.zeros(self.num_items, dtype=torch.float32, device=dev)
        self._w = torch.zeros(self.num_items, dtype=torch.int32, device=dev)
        self._draw_items = torch.zeros(4 * self.max_deg, dtype=torch.int32, device=dev)
        self._draw_r = torch.zeros(4 * self.max_deg, dtype=torch.float32, device=dev)
        self._hdr = torch.zeros(4, dtype=torch.float32, device=dev)
        self._version = 0                                      # bumped by every G step: the scorer's tables are G's
        self._fact = None                                      # (version, [P | 1], [Q | b])
        self._gemm = None                                      # [the scoring GEMM, the version its items were prepared at]
        self._last_user = None

    # ------------------------------------------------------------------ plumbing
    def _args(self):
        a, T = IrganArgs(), self.T
        a.Pg, a.Qg, a.bg, a.Pd, a.Qd, a.bd = (T[k].data_ptr() for k in NAMES)
        a.indptr, a.indices = self.csr.indptr.data_ptr(), self.csr.indices.data_ptr()
        a.z, a.w, a.draw_items, a.draw_r = (t.data_ptr() for t in (self._z, self._w, self._draw_items, self._draw_r))
        a.hdr, a.ws, a.ws_floats = self._hdr.data_ptr(), self._ws.data_ptr(), self._ws.numel()
        a.n_users, a.n_items, a.d, a.max_deg, a.max_batch = self.num_users, self.num_items, self.d, self.max_deg, MAX_BATCH
        a.lr, a.g_reg, a.d_reg, a.seed = self.lr, self.g_reg, self.d_reg, self.seed
        return a

    def _users(self, users):
        h = _ids(users)
        if len(h) and (h.min() < 0 or h.max() >= self.num_users):
            raise ValueError("IRGAN: user ids must lie in [0, %d)" % self.num_users)
        return h

    def _items(self, items):
        h = _ids(items)
        if len(h) and (h.min() < 0 or h.max() >= self.num_items):
            raise ValueError("IRGAN: item ids must lie in [0, %d)" % self.num_items)
        return h

    def factors(self):
        """([P_g | 1] [U, d + 1], [Q_g | b_g] [I, d + 1]), made once per state of G"""
        if self._fact is None or self._fact[0] != self._version:
            P, Q, b = self.T["g_P"], self.T["g_Q"], self.T["g_b"]
            ones = torch.ones((self.num_users, 1), dtype=torch.float32, device=self.dev)
            self._fact = (self._version, torch.cat([P, ones], dim=1).contiguous(),
                          torch.cat([Q, b.reshape(-1, 1)], dim=1).contiguous())
        return self._fact[1], self._fact[2]

    def _scores(self, F):
        """the score slab [B, ld] of the factor rows F through the scoring GEMM"""
        _, items = self.factors()
        B = int(F.shape[0])
        if self._gemm is None or self._gemm[0].max_rows < B:
            self._gemm = [E.score_gemm_for(items, max(B, 1)), self._version]
        elif self._gemm[1] != self._version:
            self._gemm[0].prepare(items)
            self._gemm[1] = self._version
        return self._gemm[0](F, None)

    # ------------------------------------------------------------------ weights and draws
    def weights_of(self, logits, tau):
        """uint32 weights [B, n] of the rows of float logits [B, n]: floor(exp((z - max z) / tau) 2^31)"""
        z = f32(logits).to(self.dev).contiguous().clone()
        if z.dim() != 2 or z.shape[1] < 1:
            raise ValueError("IRGAN: the logits must be [rows, n] with n >= 1")
        call("nrhip_irgan_weights", _ptr(z), z.stride(0), int(z.shape[0]), int(z.shape[1]), float(tau), _stream())
        return z.view(torch.int32).cpu().numpy().view(np.uint32)

    def weights(self, user, tau):
        """the integer weights of one user's D-data draws at temperature tau, uint32 [I] on the host"""
        h = self._users([user])
        P1, _ = self.factors()
        S = self._scores(P1[torch.from_numpy(h.astype(np.int64)).to(self.dev)].contiguous())
        call("nrhip_irgan_weights", C.c_void_p(S.data_ptr()), S.stride(0), 1, self.num_items, float(tau), _stream())
        return S[0, :self.num_items].contiguous().view(torch.int32).cpu().numpy().view(np.uint32)

    def draws(self, w, user, pos, phase, pass_counter):
        """the draws the device makes from the uint32 weights `w` for (seed, pass_counter, phase, user): phase 0 len(pos)
        plain draws, phase 1 2 len(pos) draws of the mixture with the positives `pos` (ascending)"""
        w = np.ascontiguousarray(np.asarray(w, dtype=np.uint32).reshape(-1))
        pos = np.ascontiguousarray(np.asarray(pos, dtype=np.int32).reshape(-1))
        if phase not in (0, 1):
            raise ValueError("IRGAN: phase must be 0 (D data) or 1 (G step)")
        if len(w) < 1 or not w.any():
            raise ValueError("IRGAN: the weights must hold a non-zero entry")
        if len(pos) and (pos.min() < 0 or pos.max() >= len(w) or (np.diff(pos) <= 0).any()):
            raise ValueError("IRGAN: the positives must be ascending ids in [0, %d)" % len(w))
        user, deg = int(user), len(pos)
        if user < 0:
            raise ValueError("IRGAN: user ids must not be negative")
        n_out = deg if phase == 0 else 2 * deg
        if n_out == 0:
            return np.zeros(0, np.int32)
        dev = self.dev
        indptr = np.zeros(user + 2, np.int64)
        indptr[user + 1] = deg
        w_d = torch.from_numpy(w.view(np.int32)).to(dev)
        args = [torch.from_numpy(x).to(dev) for x in (np.asarray([user], np.int32), indptr, pos, np.zeros(1, np.int64))]
        out_u = torch.zeros(2 * deg, dtype=torch.int32, device=dev)
        out_i = torch.zeros(2 * deg, dtype=torch.int32, device=dev)
        out_y = torch.zeros(2 * deg, dtype=torch.float32, device=dev)
        call("nrhip_irgan_draws", _ptr(w_d), len(w), 1, len(w), _ptr(args[0]), _ptr(args[1]), _ptr(args[2]), _ptr(args[3]),
             int(phase), self.seed, int(pass_counter) & _MASK64, _ptr(out_u), _ptr(out_i), _ptr(out_y), _stream())
        got = out_i.cpu().numpy()
        return got[1::2].copy() if phase == 0 else got

    # ------------------------------------------------------------------ the discriminator
    def d_data(self, users=None):
        """(users, items, labels) of one D pass on the device, [2 sum deg] each: for every train user (or the given ones,
        ascending as given) in turn (u, pos_k, 1), (u, draw_k, 0).  Advances the D pass counter."""
        h = self.train_users if users is None else self._users(users)
        pas, dev = self.d_passes, self.dev
        self.d_passes += 1
        deg = self.h_deg[h]
        off = np.concatenate([[0], 2 * np.cumsum(deg)]).astype(np.int64)
        n = int(off[-1])
        out_u = torch.empty(n, dtype=torch.int32, device=dev)
        out_i = torch.empty(n, dtype=torch.int32, device=dev)
        out_y = torch.empty(n, dtype=torch.float32, device=dev)
        if n == 0:
            return out_u, out_i, out_y
        P1, _ = self.factors()
        ld = (self.num_items + 63) // 64 * 64
        block = int(max(1, min(2048, (SLAB_FLOATS - 1) // ld)))
        for lo in range(0, len(h), block):
            hb = h[lo:lo + block]
            users_d = torch.from_numpy(hb).to(dev)
            S = self._scores(P1[users_d.long()].contiguous())
            call("nrhip_irgan_weights", C.c_void_p(S.data_ptr()), S.stride(0), len(hb), self.num_items, self.d_tau,
                 _stream())
            off_d = torch.from_numpy(off[lo:lo + len(hb)].copy()).to(dev)
            call("nrhip_irgan_draws", C.c_void_p(S.data_ptr()), S.stride(0), len(hb), self.num_items, _ptr(users_d),
                 _ptr(self.csr.indptr), _ptr(self.csr.indices), _ptr(off_d), 0, self.seed, pas & _MASK64, _ptr(out_u),
                 _ptr(out_i), _ptr(out_y), _stream())
        return out_u, out_i, out_y

    def _d_run(self, users, items, labels, order, batch, loss_out):
        n = int(users.numel()) if order is None else int(order.numel())
        if n == 0:
            return
        steps = -(-n // batch)
        if loss_out is not None and (loss_out.numel() < 3 * steps or loss_out.dtype != torch.float32):
            raise ValueError("IRGAN: loss_out must hold 3 floats per step (%d steps)" % steps)
        a = self._args()
        call("nrhip_irgan_d_pass", C.byref(a), _ptr(users, torch.int32), _ptr(items, torch.int32),
             _ptr(labels, torch.float32), _ptr(order, torch.int32, allow_none=True), n, int(batch),
             _ptr(loss_out, torch.float32, allow_none=True), _stream())

    def d_step(self, users, items, labels, loss_out=None):
        """one d_updates run on the triples (host arrays): moves D's touched rows only; B is the batch's own length.
        loss_out: 3 device floats (cross entropy sum, the regulariser of the rows, that of the biases), from before the
        update.  An empty batch is a no-op."""
        hu, hi = self._users(users), self._items(items)
        hy = np.ascontiguousarray(np.asarray(labels, dtype=np.float32).reshape(-1))
        if not len(hu) == len(hi) == len(hy):
            raise ValueError("IRGAN: users, items and labels must have one length")
        if len(hu) > MAX_BATCH:
            raise ValueError("IRGAN: a batch of %d pairs, the engine takes up to %d" % (len(hu), MAX_BATCH))
        if len(hu) == 0:
            return
        dev = self.dev
        self._d_run(torch.from_numpy(hu).to(dev), torch.from_numpy(hi).to(dev), torch.from_numpy(hy).to(dev), None,
                    len(hu), loss_out)

    def d_pass(self, order, loss_out=None, data=None):
        """one training_discriminator(): new data (or `data`, device triples), then the batches of `batch_size` along the
        shuffled index array `order` (a permutation of the triples' indices), the last one short; one call, no return
        to Python between the steps.  Returns the data."""
        users, items, labels = self.d_data() if data is None else data
        h = _ids(order)
        n = int(users.numel())
        if len(h) != n or (n and (h.min() < 0 or h.max() >= n)):
            raise ValueError("IRGAN: the order must index the pass's %d triples" % n)
        self._d_run(users, items, labels, torch.from_numpy(h).to(self.dev), self.batch_size, loss_out)
        return users, items, labels

    def d_pass_size(self):
        """the number of triples of a D pass: 2 sum of deg over the train users"""
        return 2 * int(self.h_deg[self.train_users].sum())

    # ------------------------------------------------------------------ the generator
    def g_step(self, user, samples=None):
        """one generator step for `user` (a train user or not; one without a train item is a no-op).  samples: 2 deg(u)
        recorded draws in place of made ones.  Made draws use the current G pass counter, which g_step leaves alone."""
        h = self._users([user])
        deg = int(self.h_deg[h[0]])
        if deg == 0:
            return
        given = None
        if samples is not None:
            s = self._items(samples)
            if len(s) != 2 * deg:
                raise ValueError("IRGAN: %d samples for user %d, 2 deg = %d expected" % (len(s), h[0], 2 * deg))
            given = torch.from_numpy(s).to(self.dev)
        a = self._args()
        call("nrhip_irgan_g_pass", C.byref(a), h.ctypes.data_as(C.c_void_p), 1, _ptr(given, allow_none=True),
             self.g_passes & _MASK64, _stream())
        self._version += 1
        self._last_user = int(h[0])

    def g_users(self, users):
        """the user steps of `users` (each with a train item) one after the other in the order given, one C call, under
        the current G pass counter"""
        h = self._users(users)
        if len(h) == 0:
            return
        if (self.h_deg[h] == 0).any():
            raise ValueError("IRGAN: a generator step needs a user with a train item")
        a = self._args()
        call("nrhip_irgan_g_pass", C.byref(a), h.ctypes.data_as(C.c_void_p), len(h), C.c_void_p(0),
             self.g_passes & _MASK64, _stream())
        self._version += 1
        self._last_user = int(h[-1])

    def g_pass(self):
        """one training_generator(): every train user in ascending id, one C call.  Advances the G pass counter."""
        self.g_users(self.train_users)
        self.g_passes += 1

    def last_weights(self):
        """uint32 [I]: the weights the last G step's draws were made from"""
        return self._w.cpu().numpy().view(np.uint32)

    def last_draws(self):
        """(items, rewards) of the last G step in draw order: int32 [2 deg], float32 [2 deg]"""
        if self._last_user is None:
            return np.zeros(0, np.int32), np.zeros(0, np.float32)
        S = 2 * int(self.h_deg[self._last_user])
        return self._draw_items[:S].cpu().numpy(), self._draw_r[:S].cpu().numpy()

    # ------------------------------------------------------------------ scoring
    def score(self, users):
        """S [B, num_items] float32 on the device: P_g[users] Q_g^T + b_g (IRGAN.py:241-246)"""
        h = self._users(users)
        if len(h) == 0:
            return torch.empty((0, self.num_items), dtype=torch.float32, device=self.dev)
        P1, _ = self.factors()
        return self._scores(P1[torch.from_numpy(h.astype(np.int64)).to(self.dev)].contiguous())[:, :self.num_items]

    def forward(self, users, items, sizes=None):
        """candidate mode: the scores of the flat `items`, sizes[b] of them for users[b] (None: one each)"""
        hu, it = self._users(users), self._items(items)
        sizes = np.ones(len(hu), np.int64) if sizes is None else np.asarray(sizes, dtype=np.int64)
        if int(sizes.sum()) != len(it) or len(sizes) != len(hu):
            raise ValueError("sizes must hold one count per user and sum to the number of items")
        out = torch.empty(len(it), dtype=torch.float32, device=self.dev)
        if len(it) == 0:
            return out
        P1, Q1 = self.factors()
        rows = torch.from_numpy(np.repeat(hu, sizes).astype(np.int32)).to(self.dev)
        call("nrhip_cfgan_pairs", _ptr(P1), P1.stride(0), _ptr(Q1), Q1.stride(0), self.d + 1, _ptr(rows),
             _ptr(torch.from_numpy(it).to(self.dev)), len(it), _ptr(out), _stream())
        return out

    def tables(self):
        """{name: numpy copy} of the six tables"""
        return {k: self.T[k].cpu().numpy() for k in NAMES}
