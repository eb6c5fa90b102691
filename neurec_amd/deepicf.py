"""DeepICF on the HIP engine: the graph of DeepICF.py:112-178 and one `sess.run((loss, optimizer))` per step, and
predict() (csrc/deepicf.hip).

DeepICF is NAIS's attention pooling (neurec_amd/nais.py: the instances, the reference's mask, the ragged buffer, the
walks) with the inner product p . q replaced by a relu tower over x0 = (num_idx^alpha p) (.) q, a batch norm in front
of every relu when `batch_norm` is on, and tf.losses.log_loss on sigmoid(out + bias[item]).

Optimiser forms, as the stand-in's trace of the reference class records them: `bias` alone is read through
embedding_lookup only — the sparse application; every other variable is dense.  `embedding_Q` and `c1` are dense
because the loss regularises the WHOLE tables (`q_application="dense"` of HistoryEngine).

Batch norm is tf.contrib.layers.batch_norm(decay=0.9, epsilon=0.001) as TF-1.12 runs it on a rank-2 input (the fused
path): training normalises with the batch mean and the biased batch variance and moves `mm[k]` / `mv[k]` by
v -= (v - batch) * 0.1, the variance entering with Bessel's correction N / max(N - 1, 1) (`bessel=False`: without).
`score()` reads the moving statistics and changes nothing.  With batch norm on, the gradient of a pre-norm bias b_k is
zero in exact arithmetic; the device writes exact zeros, so b_k never moves (Adam would amplify the rounding noise).
"""
import ctypes as C

import numpy as np
import torch

from ._lib import DEEPICF_MAX_LAYERS, DeepicfScoresArgs, DeepicfStepArgs, DeepicfTower, call
from .engine import _ptr, _stream
from .nais import NAISEngine
from .row_learner import f32

MAX_LAYERS = DEEPICF_MAX_LAYERS   # NRHIP_DEEPICF_MAX_LAYERS
MAX_WIDTH = 128                   # NRHIP_DEEPICF_MAX_WIDTH
MFMA_MAX_WIDTH = 64               # the widths (and embedding_size) the matrix-core tower of score() takes
BN_EPS = 0.001


def check_layers(layers):
    """the stated limits of the tower: NotImplementedError beyond them"""
    layers = [int(n) for n in layers]
    if not 1 <= len(layers) <= MAX_LAYERS:
        raise NotImplementedError("DeepICF: %d layers are not supported (1 to %d)" % (len(layers), MAX_LAYERS))
    for n in layers:
        if n < 1 or n > MAX_WIDTH:
            raise NotImplementedError("DeepICF: a layer of width %d is not supported (1 to %d)" % (n, MAX_WIDTH))
    return layers


class DeepICFEngine(NAISEngine):
    """Tables c1 / Q / bias / W / b / h / Wout / bout / W<k> / b<k> [/ beta<k> / gamma<k>], their optimiser state and
    gradient buffers in HBM, and the moving statistics `mm[k]`, `mv[k]` (device tensors; read or assign them).

    `step(users, items, labels, loss_out)`: one batch of the device instance stream, as NAISEngine.step.
    `gradients(...)` / `apply()`: its two halves.  `score(users)` -> [B, I] on the device: predict()."""
    NAME, ARGS, STEP = "DeepICF", DeepicfStepArgs, "nrhip_deepicf_step"

    def __init__(self, c1, Q, W, b, tower, train, lr, regs, regw, alpha, beta, max_batch, algorithm=1, activation=None,
                 batch_norm=True, learner="adam", bias=None, h=None, momentum=0.9, attention_mask="reference",
                 bessel=True, q_application="dense", pair_kernel="auto"):
        """tower: {"W<k>": [in, width], "b<k>": [width]} per layer, "Wout": [width, 1], "bout": [1], and optionally
        "beta<k>" / "gamma<k>" (zeros / ones) and "mm<k>" / "mv<k>" (zeros / ones)"""
        if pair_kernel not in ("auto", "valu", "mfma"):
            raise ValueError("pair_kernel is 'auto', 'valu' or 'mfma', got %r" % (pair_kernel,))
        L = 0
        while "W%d" % L in tower:
            L += 1
        layers = check_layers([np.shape(tower["W%d" % k])[1] for k in range(L)])
        self.layers, self.batch_norm, self.bessel = layers, bool(batch_norm), bool(bessel)

        def more(d):
            out, n_in = {}, d
            out["Wout"], out["bout"] = f32(tower["Wout"]).reshape(-1), f32(tower["bout"]).reshape(-1)
            if out["Wout"].numel() != layers[-1] or out["bout"].numel() != 1:
                raise ValueError("Wout must be [%d, 1] and bout [1]" % layers[-1])
            for k, n in enumerate(layers):
                Wk, bk = f32(tower["W%d" % k]), f32(tower["b%d" % k]).reshape(-1)
                if tuple(Wk.shape) != (n_in, n) or bk.numel() != n:
                    raise ValueError("W%d must be [%d, %d] and b%d [%d]" % (k, n_in, n, k, n))
                out["W%d" % k], out["b%d" % k] = Wk, bk
                n_in = n
            if self.batch_norm:
                for k, n in enumerate(layers):
                    out["beta%d" % k] = f32(tower["beta%d" % k]).reshape(-1) if "beta%d" % k in tower else \
                        torch.zeros(n)
                    out["gamma%d" % k] = f32(tower["gamma%d" % k]).reshape(-1) if "gamma%d" % k in tower else \
                        torch.ones(n)
                    if out["beta%d" % k].numel() != n or out["gamma%d" % k].numel() != n:
                        raise ValueError("beta%d and gamma%d must hold %d entries" % (k, k, n))
            return out
        NAISEngine.__init__(self, c1, Q, W, b, train, lr, (0.0, 0.0, 0.0), alpha, beta, max_batch, algorithm=algorithm,
                            activation=activation, loss="cross_entropy", pairwise=False, learner=learner, bias=bias,
                            h=h, momentum=momentum, attention_mask=attention_mask, c1_application="dense",
                            c1_path="walk", pair_kernel="auto", more_dense=more, q_application=q_application)
        dev = self.c1.device
        self._shared_names = self._names[:6]
        self.regs = tuple(float(x) for x in regs)
        if len(self.regs) != 3:
            raise ValueError("regs holds three entries")
        # DeepICF.py:176-178: regw[k] on layer k for k < min(len(layers), len(regw)) where regw[k] > 0
        self.regw = [float(regw[k]) if k < len(regw) and float(regw[k]) > 0 else 0.0 for k in range(len(layers))]
        self.mm = [f32(tower["mm%d" % k]).reshape(-1).to(dev) if "mm%d" % k in tower else torch.zeros(n, device=dev)
                   for k, n in enumerate(layers)] if self.batch_norm else []
        self.mv = [f32(tower["mv%d" % k]).reshape(-1).to(dev) if "mv%d" % k in tower else torch.ones(n, device=dev)
                   for k, n in enumerate(layers)] if self.batch_norm else []
        mfma_ok = max(layers + [self.d]) <= MFMA_MAX_WIDTH
        if pair_kernel == "mfma" and not mfma_ok:
            raise NotImplementedError("DeepICF: the matrix-core tower of score() takes widths and embedding_size up to "
                                      "%d" % MFMA_MAX_WIDTH)
        self.tower_mfma = mfma_ok and pair_kernel != "valu"
        floats = C.c_size_t(0)
        call("nrhip_deepicf_workspace_floats", C.byref(self._tower()), self.d, max(self.max_batch, 1), C.byref(floats))
        self._ws = torch.empty(int(floats.value), dtype=torch.float32, device=dev)

    def _tower(self):
        t = DeepicfTower()
        t.n_layers, t.batch_norm = len(self.layers), int(self.batch_norm)
        for k, n in enumerate(self.layers):
            t.width[k] = n
            t.W[k], t.b[k] = getattr(self, "W%d" % k).data_ptr(), getattr(self, "b%d" % k).data_ptr()
            if self.batch_norm:
                t.gamma[k], t.beta[k] = getattr(self, "gamma%d" % k).data_ptr(), getattr(self, "beta%d" % k).data_ptr()
                for t_ in (self.mm[k], self.mv[k]):
                    if t_.dtype != torch.float32 or t_.numel() != n or not t_.is_contiguous() or \
                            t_.device != self.c1.device:
                        raise ValueError("mm[%d] / mv[%d] must be contiguous float32 device tensors of %d entries"
                                         % (k, k, n))
                t.mm[k], t.mv[k] = self.mm[k].data_ptr(), self.mv[k].data_ptr()
        t.Wout, t.bout = self.Wout.data_ptr(), self.bout.data_ptr()
        return t

    def _shared(self, A):
        return A.nais

    def _fill(self, A):
        NAISEngine._fill(self, A.nais)
        A.tower = self._tower()
        for k in range(len(self.layers)):
            A.G_W[k], A.G_b[k] = self.G["W%d" % k].data_ptr(), self.G["b%d" % k].data_ptr()
            if self.batch_norm:
                A.G_gamma[k], A.G_beta[k] = self.G["gamma%d" % k].data_ptr(), self.G["beta%d" % k].data_ptr()
            A.regw[k] = self.regw[k]
        A.G_Wout, A.G_bout, A.ws = self.G["Wout"].data_ptr(), self.G["bout"].data_ptr(), self._ws.data_ptr()
        for k in range(3):
            A.regs[k] = self.regs[k]
        A.bessel = int(self.bessel)

    # ------------------------------------------------------------------ scoring
    def folded_tower(self):
        """the tower at inference as one affine map per layer, the moving statistics folded in on the host in
        float64: (the packed float32 array nrhip_deepicf_scores takes, the 32-tiles of every width).  The tower's
        variables reach the host in ONE copy."""
        names = ["Wout", "bout"]
        for k in range(len(self.layers)):
            names += ["W%d" % k, "b%d" % k] + (["gamma%d" % k, "beta%d" % k] if self.batch_norm else [])
        parts = [getattr(self, n) for n in names]
        if self.batch_norm:
            L = range(len(self.layers))
            names += ["mm%d" % k for k in L] + ["mv%d" % k for k in L]
            parts += list(self.mm) + list(self.mv)
        flat = torch.cat([t.detach().reshape(-1) for t in parts]).cpu().numpy().astype(np.float64)
        V, o = {}, 0
        for n, t in zip(names, parts):
            V[n] = flat[o:o + t.numel()].reshape(tuple(t.shape))
            o += t.numel()
        widths = [self.d] + self.layers
        tiles = [(n + 31) // 32 for n in widths]
        out = []
        for k, n in enumerate(self.layers):
            Wk, bk = V["W%d" % k], V["b%d" % k]
            if self.batch_norm:
                s = V["gamma%d" % k] / np.sqrt(V["mv%d" % k] + BN_EPS)
                Wk, bk = Wk * s[None, :], (bk - V["mm%d" % k]) * s + V["beta%d" % k]
            Wp = np.zeros((32 * tiles[k], 32 * tiles[k + 1]))
            Wp[:widths[k], :n] = Wk
            bp = np.zeros(32 * tiles[k + 1])
            bp[:n] = bk
            out += [Wp.reshape(-1), bp]
        wo = np.zeros(32 * tiles[-1])
        wo[:self.layers[-1]] = V["Wout"]
        out += [wo, V["bout"]]
        return np.concatenate(out).astype(np.float32), tiles

    def _scores_call(self, a, wpad, tiles):
        A = DeepicfScoresArgs()
        A.nais = a
        A.wpad, A.n_layers, A.mfma, A.wtotal = wpad.data_ptr(), len(self.layers), int(self.tower_mfma), wpad.numel()
        for k, t in enumerate(tiles):
            A.tiles[k] = t
        call("nrhip_deepicf_scores", C.byref(A), _stream())

    def score(self, users):
        """S [B, I] float32 on the device: DeepICF.py:246-258 for `users`, every item, own items included; a user
        without train items scores through an empty pooling.  Reads the moving statistics, changes nothing."""
        host, tiles = self.folded_tower()
        wpad = torch.from_numpy(host).to(self.c1.device)
        return NAISEngine.score(self, users, call=lambda a: self._scores_call(a, wpad, tiles))
