"""GRU4Rec on the HIP engine: the graph of model/sequential_recommender/GRU4Rec.py:74-132, one
`sess.run([update_opt, final_state])` per step with the recurrent states kept in HBM between steps, the users' final
states (_get_user_embeddings, GRU4Rec.py:179-225) and predict() (csrc/gru4rec.hip).

Variables E_in [I, n_0], Q [I, n_last], b [I] and per layer Wg [in + n, 2 n], bg [2 n], Wc [in + n, n], bc [n].  The
cell is TF-1.12's GRUCell: [r, u] = sigmoid([x, s] Wg + bg), c = act([x, r * s] Wc + bc), h = u s + (1 - u) c.  The
states are inputs of a step, never differentiated (the reference feeds them through placeholders).

Optimiser forms, as TF-1.12 picks them: E_in, Q and b are read through gathers only — Adam's sparse form (every row
swept, duplicates summed first); the cells' variables — ApplyAdam.
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from ._lib import Gru4recStepArgs, Gru4recWeights, call
from .engine import _ptr, _stream
from .row_learner import as_ids, f32

MAX_LAYERS = 3                # NRHIP_GRU4REC_MAX_LAYERS
MAX_WIDTH = 128               # NRHIP_GRU4REC_MAX_WIDTH
MAX_BATCH = 4096              # NRHIP_GRU4REC_MAX_BATCH
TILE = 16                     # NRHIP_GRU4REC_TILE: users per workgroup of the sequence kernel
HIDDEN_ACTS = {"tanh": 0, "relu": 1}
FINAL_ACTS = {"linear": 0, "relu": 1, "leaky_relu": 2}
LOSSES = {"top1": 0, "bpr": 1}
_ROWS = ("E_in", "Q", "b")
_CELL = ("Wg", "bg", "Wc", "bc")


class GRU4RecEngine:
    """Tables, optimiser slots, gradient buffers and the recurrent states [max_batch, n_l] in HBM.

    `step(X, Y, loss_out, reset=None)`: one batch of the session-parallel loop — gradients, Adam, then the new states
    become the states and the slots whose `reset` byte is set start from zero.  `run_schedule` issues a whole epoch.
    `user_states()` runs every user's train sequence through the stack; `score(users)` -> [n, I] on the device."""

    def __init__(self, E_in, Q, b, cells, lr, reg, max_batch, loss="top1", hidden_act="tanh", final_act="linear"):
        if hidden_act not in HIDDEN_ACTS:
            raise ValueError("There is not hidden_act named '%s'." % hidden_act)       # GRU4Rec.py:34
        if final_act not in FINAL_ACTS:
            raise ValueError("There is not final_act named '%s'." % final_act)         # GRU4Rec.py:44
        if loss not in LOSSES:
            raise ValueError("There is not loss named '%s'." % loss)                   # GRU4Rec.py:51
        cells = [tuple(f32(t) for t in c) for c in cells]
        if not 1 <= len(cells) <= MAX_LAYERS:
            raise NotImplementedError("GRU4Rec: %d layers are not supported (1 to %d)" % (len(cells), MAX_LAYERS))
        E_in, Q, b = f32(E_in), f32(Q), f32(b).reshape(-1)
        if E_in.dim() != 2 or Q.dim() != 2 or Q.shape[0] != E_in.shape[0] or b.numel() != E_in.shape[0]:
            raise ValueError("E_in must be [num_items, layers[0]], Q [num_items, layers[-1]], b [num_items]")
        layers = [int(c[1].numel()) // 2 for c in cells]
        for n in layers:
            if not 1 <= n <= MAX_WIDTH:
                raise NotImplementedError("GRU4Rec: layer width %d is not supported (1 to %d)" % (n, MAX_WIDTH))
        n_in = int(E_in.shape[1])
        if n_in != layers[0] or int(Q.shape[1]) != layers[-1]:
            raise ValueError("E_in must be [num_items, layers[0]], Q [num_items, layers[-1]], b [num_items]")
        fixed = []
        for l, ((Wg, bg, Wc, bc), n) in enumerate(zip(cells, layers)):
            if tuple(Wg.shape) != (n_in + n, 2 * n) or tuple(Wc.shape) != (n_in + n, n) or bg.numel() != 2 * n or \
                    bc.numel() != n:
                raise ValueError("layer %d: Wg must be [in + n, 2 n], bg [2 n], Wc [in + n, n], bc [n]" % l)
            fixed.append((Wg, bg.reshape(-1), Wc, bc.reshape(-1)))
            n_in = n
        max_batch = int(max_batch)
        if max_batch < 1:
            raise ValueError("max_batch must be at least 1")
        if max_batch > MAX_BATCH:
            raise NotImplementedError("GRU4Rec: max_batch=%d is not supported (1 to %d)" % (max_batch, MAX_BATCH))
        dev = E.require_gpu()
        self.loss, self.hidden_act, self.final_act = loss, hidden_act, final_act
        self.layers, self.n_layers, self.n_items, self.max_batch = layers, len(layers), int(E_in.shape[0]), max_batch
        self.lr, self.reg = float(lr), float(reg)
        self.E_in, self.Q, self.b = (t.contiguous().to(dev) for t in (E_in, Q, b))
        self.cells = [tuple(t.contiguous().to(dev) for t in c) for c in fixed]
        self.adam = E.AdamState(lr)
        tensors = self._tensors()
        self.G = {k: torch.zeros_like(t) for k, t in tensors.items()}
        self.m = {k: torch.zeros_like(t) for k, t in tensors.items()}
        self.v = {k: torch.zeros_like(t) for k, t in tensors.items()}
        self.states = [torch.zeros((max_batch, n), dtype=torch.float32, device=dev) for n in layers]
        self.h_new = [torch.zeros((max_batch, n), dtype=torch.float32, device=dev) for n in layers]
        self._keys = torch.empty(2 * max_batch, dtype=torch.int64, device=dev)
        floats = C.c_size_t(0)
        self._widths = (C.c_int * self.n_layers)(*layers)
        call("nrhip_gru4rec_workspace_floats", self.n_layers, self._widths, max_batch, C.byref(floats))
        self._ws = torch.empty(max(int(floats.value), 1), dtype=torch.float32, device=dev)
        self.t = 0
        self._seq = None
        self.H = None

    def _tensors(self):
        out = {"E_in": self.E_in, "Q": self.Q, "b": self.b}
        for l, c in enumerate(self.cells):
            for name, t in zip(_CELL, c):
                out["%s%d" % (name, l)] = t
        return out

    def tables(self):
        """{name: tensor} of every variable, in creation order: E_in, Q, b, then Wg<l>, bg<l>, Wc<l>, bc<l> per layer"""
        return self._tensors()

    def _weights(self):
        w = Gru4recWeights()
        for l, c in enumerate(self.cells):
            w.Wg[l], w.bg[l], w.Wc[l], w.bc[l] = (t.data_ptr() for t in c)
            w.width[l] = self.layers[l]
        w.n_layers, w.hidden_act = self.n_layers, HIDDEN_ACTS[self.hidden_act]
        return w

    # ------------------------------------------------------------------ training
    def reset_states(self):
        for s in self.states:
            s.zero_()

    def gradients(self, X, Y, loss_out):
        """the C call alone: loss_out, the new states (h_new[l][:B]), the dense gradients whole and the batch's rows of
        G_E_in / G_Q / G_b; no table and no state moves.  An empty batch is no work: nothing is launched and loss_out
        is set to zero."""
        B = int(X.numel())
        if B > self.max_batch:
            raise ValueError("batch larger than max_batch")
        if Y.numel() != B:
            raise ValueError("X and Y must have the same length")
        if B == 0:
            loss_out.zero_()
            return
        a = Gru4recStepArgs()
        a.Ein, a.Q, a.b = _ptr(self.E_in), _ptr(self.Q), _ptr(self.b)
        a.w = self._weights()
        a.G_Ein, a.G_Q, a.G_b = _ptr(self.G["E_in"]), _ptr(self.G["Q"]), _ptr(self.G["b"])
        for l in range(self.n_layers):
            for name in _CELL:
                getattr(a, "G_" + name)[l] = self.G["%s%d" % (name, l)].data_ptr()
            a.state[l], a.h_new[l] = self.states[l].data_ptr(), self.h_new[l].data_ptr()
        a.X, a.Y = _ptr(X, torch.int32), _ptr(Y, torch.int32)
        a.keys, a.ws, a.loss2 = _ptr(self._keys), _ptr(self._ws), _ptr(loss_out, torch.float32)
        a.n_items, a.batch = self.n_items, B
        a.final_act, a.loss_kind, a.reg = FINAL_ACTS[self.final_act], LOSSES[self.loss], self.reg
        call("nrhip_gru4rec_step", C.byref(a), _stream())

    def apply(self):
        """three sparse applications and one dense launch for the cells' variables; the gradient buffers are zero again
        afterwards"""
        for k in _ROWS:
            E.adam_sparse(getattr(self, k), self.m[k], self.v[k], self.G[k], self.adam)
        dense = []
        for l, c in enumerate(self.cells):
            for name, t in zip(_CELL, c):
                k = "%s%d" % (name, l)
                dense.append((t, self.m[k], self.v[k], self.G[k], True))
        E.adam_dense_multi(dense, self.adam)
        self.adam.advance()
        self.t += 1
        self.H = None                 # the kept user states belong to the tables before this step

    def advance(self, B, reset=None):
        """states[:B] = h_new[:B], then the rows whose byte of `reset` (uint8 [B] on the device) is set are zeroed"""
        if B == 0:
            return
        if reset is not None and reset.numel() != B:
            raise ValueError("reset must hold one byte per slot")
        L = self.n_layers
        st = (C.c_void_p * L)(*[s.data_ptr() for s in self.states])
        hn = (C.c_void_p * L)(*[h.data_ptr() for h in self.h_new])
        call("nrhip_gru4rec_advance", st, hn, self._widths, L, B, _ptr(reset, torch.uint8, allow_none=True), _stream())

    def step(self, X, Y, loss_out, reset=None):
        """loss_out: 2 floats on the device, (loss term, regulariser term) of the batch before the update.  An empty
        batch moves nothing, the step counter included."""
        self.gradients(X, Y, loss_out)
        B = int(X.numel())
        if B:
            self.apply()
            self.advance(B, reset)

    def run_schedule(self, X, Y, reset, losses):
        """a whole epoch: X, Y int32 [S, B], reset uint8 [S, B] (the slots zeroed after step s), losses float32 [S, 2]
        on the device, or host arrays that are uploaded once; no host round trip between the steps.  The items of host
        arrays are checked against the table here; device tensors are not read back (the kernels give an id that
        is no table row a row of zeros and drop its gradient, include/neurec_hip.h)"""
        for name, a in (("X", X), ("Y", Y)):
            if not isinstance(a, torch.Tensor) and np.size(a) and (np.min(a) < 0 or np.max(a) >= self.n_items):
                raise ValueError("GRU4Rec: %s holds an item outside [0, %d)" % (name, self.n_items))
        dev = self.E_in.device
        up = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        X, Y = as_ids(X, dev), as_ids(Y, dev)
        reset = up(reset).to(dev, torch.uint8).contiguous()
        if X.dim() != 2 or X.shape != Y.shape or X.shape != reset.shape or losses.shape[0] < X.shape[0]:
            raise ValueError("X, Y and reset must be [steps, batch], losses [steps, 2]")
        for s in range(int(X.shape[0])):
            self.step(X[s], Y[s], losses[s], reset[s])
        return losses

    # ------------------------------------------------------------------ the users' states and scoring
    def set_sequences(self, seq_ptr, seq):
        """every user's train items in time order: seq[seq_ptr[u]:seq_ptr[u + 1]].  The users are sorted by descending
        length once: lengths do not change during training."""
        seq_ptr = np.ascontiguousarray(seq_ptr, dtype=np.int64)
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        if seq_ptr.ndim != 1 or len(seq_ptr) < 1 or seq_ptr[0] != 0 or seq_ptr[-1] != len(seq) or \
                (np.diff(seq_ptr) < 0).any():
            raise ValueError("seq_ptr must rise from 0 to len(seq)")
        dev = self.E_in.device
        lens = np.diff(seq_ptr)
        order = np.argsort(-lens, kind="stable").astype(np.int32)
        self._seq = dict(ptr=torch.from_numpy(seq_ptr).to(dev), seq=torch.from_numpy(seq).to(dev), lens=lens,
                         n_users=len(seq_ptr) - 1, order=torch.from_numpy(order).to(dev))

    def user_states(self, users=None):
        """H [n, n_last]: the top layer's output after each listed user's whole sequence, from a zero state (None: every
        user, and the result is kept for score() / eval_factors()).  A user without items gets zeros."""
        if self._seq is None:
            raise ValueError("set_sequences() first")
        s = self._seq
        dev = self.E_in.device
        if users is None:
            order, n = s["order"], s["n_users"]
            out_row = order
        else:
            users = np.ascontiguousarray(users, dtype=np.int32).reshape(-1)
            n = len(users)
            inside = (users >= 0) & (users < s["n_users"])
            lens = np.zeros(n, np.int64)
            lens[inside] = s["lens"][users[inside]]
            perm = np.argsort(-lens, kind="stable").astype(np.int32)
            order = torch.from_numpy(users[perm]).to(dev)
            out_row = torch.from_numpy(perm).to(dev)
        H = torch.zeros((n, self.layers[-1]), dtype=torch.float32, device=dev)
        w = self._weights()
        call("nrhip_gru4rec_user_states", _ptr(s["ptr"], torch.int64), _ptr(s["seq"], torch.int32, allow_none=True)
             if s["seq"].numel() else C.c_void_p(0), s["n_users"], self.n_items,
             _ptr(order, torch.int32) if n else C.c_void_p(0), _ptr(out_row, torch.int32) if n else C.c_void_p(0), n,
             _ptr(self.E_in), C.byref(w), C.c_void_p(H.data_ptr()) if n else C.c_void_p(0), H.stride(0) if n else
             self.layers[-1], _stream())
        if users is None:
            self.H = H
        return H

    def eval_factors(self):
        """linear final_act: ([H | 1], [Q | b]) — their inner products are predict()'s scores; otherwise None"""
        if self.final_act != "linear":
            return None
        if self.H is None:
            self.user_states()
        one = torch.ones((self.H.shape[0], 1), dtype=torch.float32, device=self.H.device)
        return (torch.cat([self.H, one], dim=1).contiguous(), torch.cat([self.Q, self.b[:, None]], dim=1).contiguous())

    def score_rows(self, H, out=None):
        """S [n, I] = final_act(H Q^T + b) for the rows H [n, n_last]; `out` may be a [n, >= I] buffer"""
        n, I = int(H.shape[0]), self.n_items
        if H.dim() != 2 or H.shape[1] != self.layers[-1] or H.stride(1) != 1 and n:
            raise ValueError("H must be [n, layers[-1]] with unit column stride")
        if out is None:
            out = torch.empty((n, I), dtype=torch.float32, device=self.E_in.device)
        elif out.dim() != 2 or out.shape[0] != n or out.shape[1] < I or out.stride(1) != 1:
            raise ValueError("out must be [n, >= num_items] with unit column stride")
        call("nrhip_gru4rec_scores", C.c_void_p(H.data_ptr()) if n else None, H.stride(0) if n else self.layers[-1],
             _ptr(self.Q), _ptr(self.b), n, I, self.layers[-1], FINAL_ACTS[self.final_act],
             C.c_void_p(out.data_ptr()) if n and I else None, out.stride(0) if n else max(I, 1), _stream())
        return out

    def score(self, users):
        """S [n, I] float32 on the device: GRU4Rec.py:232-246 for `users` from the kept states of user_states()"""
        if self.H is None:
            self.user_states()
        users = torch.as_tensor(np.asarray(users, dtype=np.int64), device=self.H.device)
        return self.score_rows(self.H.index_select(0, users).contiguous())
