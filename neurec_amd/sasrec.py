"""SASRec on the HIP engine: the graph of model/sequential_recommender/SASRec.py:311-383, one
`sess.run(self.train_opt)` per step, and predict() (csrc/sasrec.hip).

Variables in creation order: item_emb [I, d], pos_emb [L, d]; per block ln1 (beta, gamma), Wq, bq, Wk, bk, Wv, bv, ln2
(beta, gamma), W1, b1, W2, b2 (the conv1d kernels [1, d, d] are kept as [d, d]); the final ln (beta, gamma).

Optimiser forms, as TF-1.12 picks them (Adam with beta2 = 0.98): item_emb is read through a concat and a scaling, so its
gradient is dense — ApplyAdam over the whole table, every row moving once its `m` is non-zero; pos_emb is gathered from
the variable — Adam's sparse form, which sweeps every row (the note in neurec_amd/gru4rec.py) — unless l2_emb != 0, when
the regulariser's dense gradient joins the gather's and TF applies ApplyAdam; everything else ApplyAdam.

Dropout: `masks` given as 1 + 3 num_blocks uint8 device tensors (the embedding [B, L, d]; per block the attention
weights [h B, L, L] head-major, the feed-forward's hidden layer and its output [B, L, d]), or a counter-based device
generator keyed by (seed, step, site, element).

A batch without any target (sum(is_target) == 0) makes the reference divide 0 by 0 and poison every variable; here that
step is skipped and counted in `skipped_steps`.
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from ._lib import SasrecStepArgs, SasrecWeights, call
from .engine import _ptr, _stream
from .row_learner import as_ids, f32

MAX_BLOCKS = 4                # NRHIP_SASREC_MAX_BLOCKS
MAX_WIDTH = 128               # NRHIP_SASREC_MAX_WIDTH
MAX_LEN = 200                 # NRHIP_SASREC_MAX_LEN
MAX_BATCH = 4096              # NRHIP_SASREC_MAX_BATCH
MAX_WEIGHTS = 1 << 30         # NRHIP_SASREC_MAX_WEIGHTS: num_heads * batch * max_len^2 saved attention weights
BETA2 = 0.98                  # SASRec.py:383
BLOCK_VARS = ("ln1_beta", "ln1_gamma", "Wq", "bq", "Wk", "bk", "Wv", "bv", "ln2_beta", "ln2_gamma", "W1", "b1", "W2",
              "b2")


def n_sites(num_blocks):
    return 1 + 3 * num_blocks


class SASRecEngine:
    """Tables, optimiser slots and gradient buffers in HBM.

    `blocks`: per block the 14 arrays of BLOCK_VARS; `final_ln`: (beta, gamma).  `step(seq, pos, neg, loss_out)`: one
    batch int32 [B, L] each, padded in front with the item id I — gradients, then Adam.  `run_schedule` issues a whole
    epoch.  `user_embeddings(users)` runs the users' train sequences with training off; `score(users)` -> [n, I] on the
    device."""

    def __init__(self, item_emb, pos_emb, blocks, final_ln, lr, l2_emb, max_batch, num_heads, dropout_rate, seed=2017):
        item_emb, pos_emb = f32(item_emb), f32(pos_emb)
        if item_emb.dim() != 2 or pos_emb.dim() != 2 or pos_emb.shape[1] != item_emb.shape[1]:
            raise ValueError("item_emb must be [num_items, hidden_units], pos_emb [max_len, hidden_units]")
        d, L, nb, h = int(item_emb.shape[1]), int(pos_emb.shape[0]), len(blocks), int(num_heads)
        max_batch = int(max_batch)
        if not 1 <= d <= MAX_WIDTH:
            raise NotImplementedError("SASRec: hidden_units=%d is not supported (1 to %d)" % (d, MAX_WIDTH))
        if not 1 <= L <= MAX_LEN:
            raise NotImplementedError("SASRec: max_len=%d is not supported (1 to %d)" % (L, MAX_LEN))
        if not 1 <= nb <= MAX_BLOCKS:
            raise NotImplementedError("SASRec: num_blocks=%d is not supported (1 to %d)" % (nb, MAX_BLOCKS))
        if h < 1 or d % h:
            raise ValueError("SASRec: num_heads=%d does not divide hidden_units=%d" % (h, d))    # tf.split raises
        if max_batch < 1:
            raise ValueError("max_batch must be at least 1")
        if max_batch > MAX_BATCH:
            raise NotImplementedError("SASRec: max_batch=%d is not supported (1 to %d)" % (max_batch, MAX_BATCH))
        if h * max_batch * L * L > MAX_WEIGHTS:
            raise NotImplementedError("SASRec: num_heads * max_batch * max_len^2 = %d saved attention weights are not "
                                      "supported (up to %d)" % (h * max_batch * L * L, MAX_WEIGHTS))
        if not 0.0 <= float(dropout_rate) < 1.0:
            raise ValueError("SASRec: dropout_rate=%r outside [0, 1)" % (dropout_rate,))
        fixed = []
        for i, blk in enumerate(blocks):
            blk = [f32(t) for t in blk]
            if len(blk) != len(BLOCK_VARS):
                raise ValueError("block %d: %d arrays, want %s" % (i, len(blk), ", ".join(BLOCK_VARS)))
            out = []
            for name, t in zip(BLOCK_VARS, blk):
                want = d * d if name.startswith("W") else d
                if t.numel() != want:
                    raise ValueError("block %d: %s holds %d values, want %d" % (i, name, t.numel(), want))
                out.append(t.reshape(d, d) if name.startswith("W") else t.reshape(d))
            fixed.append(out)
        final_ln = [f32(t).reshape(-1) for t in final_ln]
        if len(final_ln) != 2 or any(t.numel() != d for t in final_ln):
            raise ValueError("final_ln must be (beta [hidden_units], gamma [hidden_units])")
        dev = E.require_gpu()
        self.d, self.L, self.n_blocks, self.n_heads = d, L, nb, h
        self.n_items, self.max_batch = int(item_emb.shape[0]), max_batch
        self.lr, self.l2_emb, self.rate, self.seed = float(lr), float(l2_emb), float(dropout_rate), int(seed)
        self.item_emb, self.pos_emb = item_emb.contiguous().to(dev), pos_emb.contiguous().to(dev)
        self.blocks = [[t.contiguous().to(dev) for t in blk] for blk in fixed]
        self.final_ln = [t.contiguous().to(dev) for t in final_ln]
        self.adam = E.AdamState(lr, beta2=BETA2)
        tensors = self._tensors()
        self.G = {k: torch.zeros_like(t) for k, t in tensors.items()}
        self.m = {k: torch.zeros_like(t) for k, t in tensors.items()}
        self.v = {k: torch.zeros_like(t) for k, t in tensors.items()}
        self._keys = torch.empty(3 * max_batch * L, dtype=torch.int64, device=dev)
        floats = C.c_size_t(0)
        call("nrhip_sasrec_workspace_floats", max_batch, L, d, nb, h, C.byref(floats))
        self._ws = torch.empty(max(int(floats.value), 1), dtype=torch.float32, device=dev)
        self._zero_bias = torch.zeros(max(self.n_items, 1), dtype=torch.float32, device=dev)
        self.t = 0
        self.skipped_steps = 0
        self._seq = None

    def _tensors(self):
        out = {"item_emb": self.item_emb, "pos_emb": self.pos_emb}
        for i, blk in enumerate(self.blocks):
            for name, t in zip(BLOCK_VARS, blk):
                out["b%d_%s" % (i, name)] = t
        out["lnf_beta"], out["lnf_gamma"] = self.final_ln
        return out

    def tables(self):
        """{name: tensor} of every variable, in creation order"""
        return self._tensors()

    def _weights(self):
        w = SasrecWeights()
        w.item, w.pos = self.item_emb.data_ptr(), self.pos_emb.data_ptr()
        for i, blk in enumerate(self.blocks):
            for k, t in enumerate(blk):
                w.blk[i][k] = t.data_ptr()
        w.lnf_beta, w.lnf_gamma = (t.data_ptr() for t in self.final_ln)
        w.n_items, w.d, w.L, w.n_blocks, w.n_heads = self.n_items, self.d, self.L, self.n_blocks, self.n_heads
        return w

    # ------------------------------------------------------------------ inputs
    def _check_host(self, name, a):
        if not isinstance(a, torch.Tensor) and np.size(a) and (np.min(a) < 0 or np.max(a) > self.n_items):
            raise ValueError("SASRec: %s holds an item outside [0, %d]" % (name, self.n_items))

    def _ids(self, a):
        return as_ids(a, self.item_emb.device)

    # ------------------------------------------------------------------ training
    def gradients(self, seq, pos, neg, loss_out, masks=None):
        """the C call alone: loss_out (2 floats on the device: loss term, regulariser term) and every gradient whole; no
        table moves.  Host arrays are checked for ids outside [0, I].  An empty batch and a batch whose every row is
        empty are no work: nothing is launched and loss_out is set to zero.  Returns the number of targets when the
        inputs are host arrays, else None."""
        for name, a in (("seq", seq), ("pos", pos), ("neg", neg)):
            self._check_host(name, a)
        n_target = None if isinstance(pos, torch.Tensor) else int((np.asarray(pos) != self.n_items).sum())
        all_pad = not isinstance(seq, torch.Tensor) and not isinstance(pos, torch.Tensor) and \
            not (np.asarray(seq) != self.n_items).any() and n_target == 0
        seq, pos, neg = self._ids(seq), self._ids(pos), self._ids(neg)
        if seq.dim() != 2 or seq.shape[1] != self.L or pos.shape != seq.shape or neg.shape != seq.shape:
            raise ValueError("seq, pos and neg must be [batch, max_len]")
        B = int(seq.shape[0])
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if B == 0 or all_pad:
            loss_out.zero_()
            return n_target
        a = SasrecStepArgs()
        a.w = self._weights()
        a.G_item, a.G_pos = self.G["item_emb"].data_ptr(), self.G["pos_emb"].data_ptr()
        for i in range(self.n_blocks):
            for k, name in enumerate(BLOCK_VARS):
                a.G_blk[i][k] = self.G["b%d_%s" % (i, name)].data_ptr()
        a.G_lnf_beta, a.G_lnf_gamma = self.G["lnf_beta"].data_ptr(), self.G["lnf_gamma"].data_ptr()
        a.seq, a.pos_ids, a.neg_ids = _ptr(seq, torch.int32), _ptr(pos, torch.int32), _ptr(neg, torch.int32)
        if masks is not None:
            shapes = [(B, self.L, self.d)]
            for _ in range(self.n_blocks):
                shapes += [(self.n_heads * B, self.L, self.L), (B, self.L, self.d), (B, self.L, self.d)]
            if len(masks) != len(shapes):
                raise ValueError("masks: %d sites, want %d" % (len(masks), len(shapes)))
            for k, (mk, shp) in enumerate(zip(masks, shapes)):
                if tuple(mk.shape) != shp:
                    raise ValueError("masks[%d] must be %s" % (k, shp))
                a.mask[k] = _ptr(mk, torch.uint8)
        a.keys, a.ws, a.loss2 = _ptr(self._keys), _ptr(self._ws), _ptr(loss_out, torch.float32)
        a.seed, a.batch, a.step = self.seed, B, self.t
        a.rate, a.l2_emb = self.rate, self.l2_emb
        call("nrhip_sasrec_step", C.byref(a), _stream())
        return n_target

    def apply(self):
        """pos_emb in the sparse form (ApplyAdam when it has a regulariser), one dense launch for everything else; the
        gradient buffers are zero again afterwards"""
        dense = []
        for k, t in self._tensors().items():
            if k == "pos_emb" and self.l2_emb == 0.0:
                E.adam_sparse(t, self.m[k], self.v[k], self.G[k], self.adam)
            else:
                dense.append((t, self.m[k], self.v[k], self.G[k], True))
        E.adam_dense_multi(dense, self.adam)
        self.adam.advance()
        self.t += 1

    def _skip(self):
        for g in self.G.values():
            g.zero_()
        self.skipped_steps += 1

    def step(self, seq, pos, neg, loss_out, masks=None, n_target=None):
        """gradients, then Adam.  A batch without any target is skipped and counted (the reference divides 0 by 0
        there); an empty batch moves nothing.  The number of targets is counted on the host for host arrays; for
        device tensors it is read back once unless `n_target` is given."""
        if n_target is None and isinstance(pos, torch.Tensor):
            n_target = int((pos != self.n_items).sum().item())
        counted = self.gradients(seq, pos, neg, loss_out, masks)
        n_target = counted if n_target is None else n_target
        if int(np.shape(seq)[0] if not isinstance(seq, torch.Tensor) else seq.shape[0]) == 0:
            return
        if n_target == 0:
            self._skip()
            return
        self.apply()

    def run_schedule(self, seq, pos, neg, losses, masks=None):
        """a whole epoch: seq, pos, neg int32 [S, B, L], losses float32 [S, 2] on the device, or host arrays that are
        uploaded once; the targets of all steps are counted before the first one, so there is no host round trip
        between the steps.  masks: per step the list `gradients` takes, or None."""
        for name, a in (("seq", seq), ("pos", pos), ("neg", neg)):
            self._check_host(name, a)
        seq, pos, neg = self._ids(seq), self._ids(pos), self._ids(neg)
        if seq.dim() != 3 or pos.shape != seq.shape or neg.shape != seq.shape or losses.shape[0] < seq.shape[0]:
            raise ValueError("seq, pos and neg must be [steps, batch, max_len], losses [steps, 2]")
        counts = (pos != self.n_items).sum(dim=(1, 2)).cpu().numpy() if seq.shape[0] else []
        for s in range(int(seq.shape[0])):
            self.step(seq[s], pos[s], neg[s], losses[s], None if masks is None else masks[s], int(counts[s]))
        return losses

    # ------------------------------------------------------------------ the users' embeddings and scoring
    def set_sequences(self, seq_ptr, seq):
        """every user's train items in time order: seq[seq_ptr[u]:seq_ptr[u + 1]]"""
        seq_ptr = np.ascontiguousarray(seq_ptr, dtype=np.int64)
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        if seq_ptr.ndim != 1 or len(seq_ptr) < 1 or seq_ptr[0] != 0 or seq_ptr[-1] != len(seq) or \
                (np.diff(seq_ptr) < 0).any():
            raise ValueError("seq_ptr must rise from 0 to len(seq)")
        if len(seq) and (seq.min() < 0 or seq.max() >= self.n_items):
            raise ValueError("SASRec: seq holds an item outside [0, %d)" % self.n_items)
        self._seq = (seq_ptr, seq)

    def padded(self, users):
        """[n, L] int32: each user's last L train items, padded in front with I (pad_sequences 'pre' / 'pre'); a user
        without items, or outside the data, is the all-padded row"""
        if self._seq is None:
            raise ValueError("set_sequences() first")
        ptr, seq = self._seq
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        out = np.full((len(users), self.L), self.n_items, np.int32)
        for r, u in enumerate(users):
            if 0 <= u < len(ptr) - 1:
                cut = seq[max(ptr[u], ptr[u + 1] - self.L):ptr[u + 1]]
                if len(cut):
                    out[r, self.L - len(cut):] = cut
        return out

    def forward_rows(self, seq, scale=1.0):
        """scale * seq[:, -1, :] of the graph with training off, for seq int32 [n, L]"""
        self._check_host("seq", seq)
        seq = self._ids(seq)
        if seq.dim() != 2 or seq.shape[1] != self.L:
            raise ValueError("seq must be [n, max_len]")
        n = int(seq.shape[0])
        out = torch.empty((n, self.d), dtype=torch.float32, device=self.item_emb.device)
        w = self._weights()
        for lo in range(0, n, self.max_batch):
            part = seq[lo:lo + self.max_batch]
            call("nrhip_sasrec_forward", C.byref(w), _ptr(part, torch.int32), int(part.shape[0]), _ptr(self._ws),
                 float(scale), C.c_void_p(out[lo:].data_ptr()), self.d, _stream())
        return out

    def user_embeddings(self, users):
        """[n, d]: the last position of each listed user's whole train sequence, training off (SASRec.py:357, 434-437)"""
        return self.forward_rows(self.padded(users))

    def score(self, users):
        """S [n, I] float32 on the device: seq[:, -1, :] . (item_emb sqrt(d))^T (SASRec.py:386-387)"""
        return self.score_rows(self.padded(users))

    def score_rows(self, seq):
        """score() for padded rows seq int32 [n, L] given as they are"""
        H = self.forward_rows(seq, scale=float(np.sqrt(np.float32(self.d))))
        n, I = int(H.shape[0]), self.n_items
        out = torch.empty((n, I), dtype=torch.float32, device=H.device)
        call("nrhip_gru4rec_scores", C.c_void_p(H.data_ptr()) if n else None, self.d, _ptr(self.item_emb),
             _ptr(self._zero_bias), n, I, self.d, 0, C.c_void_p(out.data_ptr()) if n and I else None, max(I, 1),
             _stream())
        return out
