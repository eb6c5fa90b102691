"""SBPR on the HIP engine: the social item sets of model/social_recommender/SBPR.py:40-49, the instances of one epoch
(SBPR.py:104-106, 122-148) and one `sess.run((loss, optimizer))` per step (csrc/sbpr.hip).

An instance is (user u, train item i, social item k, negative j, suk): k an item some user trusted by u has and u has
not, suk = 1 + the number of trusted users who hold k, j outside R_u and the social set C_u.
    x_a = P_u . Q_a + b_a;   loss = f((x_i - x_k) / suk) + f(x_k - x_j) + reg l2(P_u, Q_k, Q_i, Q_j, b_i, b_k, b_j)
predict() ranks by P_u . Q_j WITHOUT the bias that training uses (SBPR.py:155-166).

The sets are the product S R of the trust matrix and the train matrix with counts, minus R's own pattern: the pairs
(u, f in S_u, k in R_f) are expanded into sort keys in blocks of whole users whose expansion fits `workspace_pairs`; a user's keys lie together,
so each user's segment is sorted on its own (the ones above `segment_pairs` keys one by one).

Optimiser forms, as TF-1.12 picks them: P, Q and b are read through embedding_lookup / tf.gather only — the sparse
application (neurec_amd/row_learner.py), b as a [num_items, 1] table.
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from ._lib import SbprSetsArgs, SbprStepArgs, SbprStreamArgs, call
from .engine import _ptr, _stream
from .row_learner import RowLearner, addr, as_ids, check_loss_learner, f32

MAX_D = 128                   # NRHIP_SBPR_MAX_D
MAX_PAIRS = 1 << 30           # NRHIP_SBPR_MAX_PAIRS
WORKSPACE_PAIRS = 1 << 23     # expanded (user, trusted user, item) pairs of one block: 24 bytes of work space each
SEGMENT_PAIRS = 16384         # NRHIP_SBPR_SEGMENT_PAIRS: a user's expansion that one workgroup sorts in its LDS
_CHUNK = 1024                 # keys per workgroup of the mark and compact kernels
_TABLES = ("P", "Q", "b")


def _csr_arrays(csr, n_rows, n_cols, what):
    """(int64 indptr, int32 indices ascending and distinct per row) of a scipy CSR matrix, or of an (indptr, indices)
    pair that is in that form already"""
    if hasattr(csr, "tocsr"):
        csr = csr.tocsr().copy()
        csr.sum_duplicates()
        csr.sort_indices()
        if csr.shape != (n_rows, n_cols):
            raise ValueError("%s must be [%d, %d], got %r" % (what, n_rows, n_cols, csr.shape))
        indptr, indices = csr.indptr, csr.indices
    else:
        indptr, indices = csr
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    if indptr.shape != (n_rows + 1,) or indptr[0] != 0 or indptr[-1] != indices.size or np.any(np.diff(indptr) < 0):
        raise ValueError("%s: bad indptr" % what)
    if indices.size and (indices.min() < 0 or indices.max() >= n_cols):
        raise ValueError("%s: a column index is outside [0, %d)" % (what, n_cols))
    inner = np.ones(indices.size, dtype=bool)
    inner[indptr[:-1][np.diff(indptr) > 0]] = False
    if np.any(np.diff(indices)[inner[1:]] <= 0):
        raise ValueError("%s: the indices of a row must be ascending and distinct" % what)
    return indptr, indices


class SBPREngine:
    """Tables P [U, d], Q [I, d], b [I], their optimiser state and gradient buffers, the train and trust CSR and the
    social sets in HBM.

    `social_sets()` -> (indptr [U + 1], items, counts) on the device; `eligible_users`: the users with a social item.
    `sample_epoch(epoch)` -> (users, items, social, negatives, suk) on the device; `step(...)` one batch of them;
    `train_epoch(epoch)` the epoch's steps from the device stream; `score(users)` -> [n, I] on the device."""

    def __init__(self, P, Q, b, train_csr, trust_csr, lr, reg_mf, max_batch, loss="bpr", learner="adam", seed=2019,
                 workspace_pairs=WORKSPACE_PAIRS, momentum=0.9, segment_pairs=SEGMENT_PAIRS):
        loss, learner, self.loss_kind = check_loss_learner(loss, learner, True)
        P, Q, b = f32(P), f32(Q), f32(b).reshape(-1)
        if P.dim() != 2 or Q.dim() != 2 or Q.shape[1] != P.shape[1]:
            raise ValueError("P must be [num_users, embedding_size], Q [num_items, embedding_size]")
        (U, d), I = P.shape, Q.shape[0]
        if d < 1 or d > MAX_D:
            raise NotImplementedError("SBPR: embedding_size=%d is not supported (1 to %d)" % (d, MAX_D))
        if b.numel() != I:
            raise ValueError("b must hold num_items entries")
        workspace_pairs = int(workspace_pairs)
        if workspace_pairs < 1 or workspace_pairs > MAX_PAIRS:
            raise ValueError("workspace_pairs must lie in 1..%d" % MAX_PAIRS)
        tr_ptr, tr_idx = _csr_arrays(train_csr, U, I, "train matrix")
        s_ptr, s_idx = _csr_arrays(trust_csr, U, U, "trust matrix")
        dev = E.require_gpu()
        self.loss, self.learner = loss, learner
        self.n_users, self.n_items, self.d = U, I, d
        self.P, self.Q, self.b = (t.contiguous().to(dev) for t in (P, Q, b))
        self.G = {k: torch.zeros_like(getattr(self, k)) for k in _TABLES}
        self.lr, self.momentum, self.reg_mf = float(lr), float(momentum), float(reg_mf)
        self.adam = E.AdamState(lr)
        self.opt = RowLearner(learner, lr, momentum, self.adam)
        slots = {k: self.opt.slots(getattr(self, k)) for k in _TABLES}
        self.s0, self.s1 = ({k: s[i] for k, s in slots.items()} for i in (0, 1))
        self.flag = {k: self.opt.flag(getattr(self, k).shape[0], dev) for k in _TABLES}
        self.max_batch = int(max_batch)
        mb = max(self.max_batch, 1)
        self._keys = torch.empty(4 * mb, dtype=torch.int64, device=dev)
        self._scal = torch.empty(4 * mb, dtype=torch.float32, device=dev)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.t = 0
        self.tr_indptr, self.tr_indices = torch.from_numpy(tr_ptr).to(dev), torch.from_numpy(tr_idx).to(dev)
        self.s_indptr, self.s_indices = torch.from_numpy(s_ptr).to(dev), torch.from_numpy(s_idx).to(dev)
        self.workspace_pairs = workspace_pairs
        self.segment_pairs = int(segment_pairs)
        if self.segment_pairs < 1 or self.segment_pairs > SEGMENT_PAIRS:
            raise ValueError("segment_pairs must lie in 1..%d" % SEGMENT_PAIRS)
        self.blocks, self.n_blocks = [], 0
        self._build_sets()
        self._build_slots(tr_ptr)

    # ------------------------------------------------------------------ the social sets
    def _build_sets(self):
        U, dev = self.n_users, self.P.device
        sizes = torch.zeros(U, dtype=torch.int64, device=dev)
        call("nrhip_sbpr_expansion_sizes", _ptr(self.tr_indptr), _ptr(self.s_indptr),
             C.c_void_p(self.s_indices.data_ptr()), U, _ptr(sizes), _stream())
        h_sizes = sizes.cpu().numpy()
        over = np.flatnonzero(h_sizes > self.workspace_pairs)
        if over.size:
            u = int(over[0])
            raise ValueError("SBPR: the trusted users of user %d hold %d items, more than the workspace of %d pairs; "
                             "raise workspace_pairs" % (u, int(h_sizes[u]), self.workspace_pairs))
        # blocks of whole users whose expansions fit the workspace: each the longest run of users that does
        csum = np.concatenate([[0], np.cumsum(h_sizes)])
        blocks, u0 = [], 0
        while u0 < U:
            u1 = int(np.searchsorted(csum, csum[u0] + self.workspace_pairs, side="right")) - 1
            blocks.append((u0, u1, int(csum[u1] - csum[u0])))
            u0 = u1
        if not blocks:
            blocks.append((0, 0, 0))
        self.blocks, self.n_blocks = blocks, len(blocks)       # (first user, end user, expanded pairs)
        W = max(max(n for _, _, n in blocks), 1)
        keys = torch.empty(W, dtype=torch.int64, device=dev)
        cnt = torch.empty(W, dtype=torch.int32, device=dev)
        pos = torch.empty(W, dtype=torch.int32, device=dev)
        chunk = torch.empty((W + _CHUNK - 1) // _CHUNK + 1, dtype=torch.int64, device=dev)
        items_ws = torch.empty(W, dtype=torch.int32, device=dev)
        counts_ws = torch.empty(W, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        ptrs, items, counts, base = [], [], [], 0
        for u0, u1, n_pairs in blocks:
            pair_off = torch.zeros(u1 - u0 + 1, dtype=torch.int64, device=dev)
            pair_off[1:] = torch.cumsum(sizes[u0:u1], 0)
            block_ptr = torch.empty(u1 - u0 + 1, dtype=torch.int64, device=dev)
            a = SbprSetsArgs()
            a.tr_indptr, a.tr_indices = _ptr(self.tr_indptr), C.c_void_p(self.tr_indices.data_ptr())
            a.s_indptr, a.s_indices = _ptr(self.s_indptr), C.c_void_p(self.s_indices.data_ptr())
            a.pair_off, a.keys, a.cnt, a.pos, a.chunk = _ptr(pair_off), _ptr(keys), _ptr(cnt), _ptr(pos), _ptr(chunk)
            a.items_out, a.counts_out = _ptr(items_ws), _ptr(counts_ws)
            a.indptr_out, a.total = _ptr(block_ptr), _ptr(total)
            a.n_users, a.n_items, a.u0, a.u1, a.n_pairs = U, self.n_items, u0, u1, n_pairs
            # a user's keys lie together: the segments one workgroup sorts in one launch, the larger ones one by one
            mine = h_sizes[u0:u1]
            big = np.flatnonzero(mine > self.segment_pairs)
            seg_len = torch.from_numpy(np.where(mine > self.segment_pairs, 0, mine).astype(np.int32)).to(dev)
            big_off = (C.c_int64 * max(len(big), 1))(*[int(csum[u0 + x] - csum[u0]) for x in big])
            big_len = (C.c_int64 * max(len(big), 1))(*[int(mine[x]) for x in big])
            a.seg_len, a.big_off, a.big_len = _ptr(seg_len), C.cast(big_off, C.c_void_p), C.cast(big_len, C.c_void_p)
            a.max_seg_len, a.n_big = int(min(self.segment_pairs, mine.max(initial=0))), len(big)
            call("nrhip_sbpr_sets_block", C.byref(a), _stream())
            n = int(total.item())
            ptrs.append(block_ptr[:-1] + base)
            items.append(items_ws[:n].clone())
            counts.append(counts_ws[:n].clone())
            base += n
        ptrs.append(torch.tensor([base], dtype=torch.int64, device=dev))
        self.c_indptr = torch.cat(ptrs).contiguous()
        self.c_items = torch.cat(items).contiguous()
        self.c_counts = torch.cat(counts).contiguous()
        n_social = self.c_indptr[1:] - self.c_indptr[:-1]
        n_train = self.tr_indptr[1:] - self.tr_indptr[:-1]
        full = torch.nonzero((n_social > 0) & (n_social + n_train >= self.n_items)).reshape(-1)
        if full.numel():
            raise ValueError("SBPR: user %d has no item outside its train items and its social items: no negative "
                             "can be drawn" % int(full[0]))
        self.eligible_users = torch.nonzero(n_social > 0).reshape(-1).to(torch.int32).contiguous()

    def social_sets(self):
        """(indptr int64 [U + 1], items int32 ascending per user, counts int32 = suk - 1) on the device"""
        return self.c_indptr, self.c_items, self.c_counts

    def _build_slots(self, tr_ptr):
        dev = self.P.device
        elig = self.eligible_users.cpu().numpy().astype(np.int64)
        deg = np.diff(tr_ptr)[elig]
        slot_ptr = np.zeros(elig.size + 1, dtype=np.int64)
        np.cumsum(deg, out=slot_ptr[1:])
        self.n_instances = int(slot_ptr[-1])
        self._slot_ptr = torch.from_numpy(slot_ptr).to(dev)
        self._slot_row = torch.from_numpy(np.repeat(np.arange(elig.size, dtype=np.int32), deg)).to(dev)

    # ------------------------------------------------------------------ the instance stream
    def sample_epoch(self, epoch, shuffle=True):
        """(users, items, social items, negatives int32 [n_instances], suk float32 [n_instances]) of `epoch` on the
        device: a pure function of (seed, epoch)"""
        n, dev = self.n_instances, self.P.device
        out = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
        suk = torch.empty(n, dtype=torch.float32, device=dev)
        if n == 0:
            return out[0], out[1], out[2], out[3], suk
        a = SbprStreamArgs()
        a.tr_indptr, a.tr_indices = _ptr(self.tr_indptr), _ptr(self.tr_indices)
        a.c_indptr, a.c_items, a.c_counts = _ptr(self.c_indptr), _ptr(self.c_items), _ptr(self.c_counts)
        a.slot_ptr, a.slot_row, a.elig = _ptr(self._slot_ptr), _ptr(self._slot_row), _ptr(self.eligible_users)
        a.users_out, a.items_out, a.social_out, a.neg_out = (_ptr(t) for t in out)
        a.suk_out = _ptr(suk)
        a.n_slots, a.out_begin, a.out_count = n, 0, n
        a.seed, a.epoch = self.seed, int(epoch) & 0xFFFFFFFFFFFFFFFF
        a.n_elig, a.n_users, a.n_items = int(self.eligible_users.numel()), self.n_users, self.n_items
        a.shuffle = int(bool(shuffle))
        call("nrhip_sbpr_stream", C.byref(a), _stream())
        return out[0], out[1], out[2], out[3], suk

    # ------------------------------------------------------------------ training
    def gradients(self, users, items, social, negatives, suk, loss_out):
        """the C call alone: loss_out and the batch's rows of G_P / G_Q / G_b (and the row flags); no table moves.  An
        empty batch is no work: nothing is launched and loss_out is set to zero."""
        B = int(users.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if items.numel() != B or social.numel() != B or negatives.numel() != B or suk.numel() != B:
            raise ValueError("users, items, social items, negatives and suk must have the same length")
        if B == 0:
            loss_out.zero_()
            return
        a = SbprStepArgs()
        for k in _TABLES:
            setattr(a, k, _ptr(getattr(self, k)))
            setattr(a, "G_" + k, _ptr(self.G[k]))
            setattr(a, "flag_" + k, addr(self.flag[k]))
        a.users, a.items = _ptr(users, torch.int32), _ptr(items, torch.int32)
        a.social, a.neg, a.suk = _ptr(social, torch.int32), _ptr(negatives, torch.int32), _ptr(suk, torch.float32)
        a.keys, a.scal, a.loss2 = _ptr(self._keys), _ptr(self._scal), _ptr(loss_out, torch.float32)
        a.n_users, a.n_items, a.d, a.batch = self.n_users, self.n_items, self.d, B
        a.loss_kind, a.reg = self.loss_kind, self.reg_mf
        call("nrhip_sbpr_step", C.byref(a), _stream())

    def apply(self):
        """three sparse applications; the gradient buffers (and flags) are zero again afterwards"""
        for k in _TABLES:
            self.opt.apply(getattr(self, k), self.s0[k], self.s1[k], self.G[k], self.flag[k])
        self.adam.advance()
        self.t += 1

    def step(self, users, items, social, negatives, suk, loss_out):
        """loss_out: 2 floats on the device, (loss term, regulariser term) of the batch before the update.  An empty
        batch moves nothing, the step counter included."""
        self.gradients(users, items, social, negatives, suk, loss_out)
        if int(users.numel()):
            self.apply()

    def train_epoch(self, epoch, batch_size=None):
        """the epoch's steps from the device stream, the last batch short; -> (the sum of the steps' losses as the
        reference adds them, the number of instances).  One copy to the host per epoch."""
        bs = self.max_batch if batch_size is None else int(batch_size)
        if bs < 1 or bs > self.max_batch:
            raise ValueError("batch_size must lie in 1..max_batch")
        fields = self.sample_epoch(epoch)
        n = self.n_instances
        steps = (n + bs - 1) // bs
        losses = torch.zeros((max(steps, 1), 2), dtype=torch.float32, device=self.P.device)
        for s in range(steps):
            lo, hi = s * bs, min(n, (s + 1) * bs)
            self.step(*(f[lo:hi] for f in fields), losses[s])
        total = 0.0
        for x, y in losses[:steps].cpu().numpy():              # `total_loss += loss`, SBPR.py:116
            total += np.float32(x) + np.float32(y)
        return total, n

    # ------------------------------------------------------------------ scoring
    def score(self, users):
        """S [n, I] float32 on the device: P_u . Q_j for `users`, every item, WITHOUT the bias (SBPR.py:155-158)"""
        users = as_ids(users, self.P.device)
        gemm = E.score_gemm_for(self.Q, max(int(users.numel()), 1))
        return gemm(self.P, users)[:, :self.n_items]
