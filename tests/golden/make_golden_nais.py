"""Golden NAIS trace produced by the REFERENCE's own NAIS class (model/general_recommender/NAIS.py).

The class is imported whole and unchanged through oracle/ref_models.py and runs under oracle/tf_shim.py, as
make_golden_fism.py does for FISM.  The call forms the shim lacks are attached here by their published definitions:
`sequence_mask`, `tile`, `reshape` and `stack` on python ints and shape entries, `ones`, and (from make_golden_fism)
`constant(value, dtype, shape)` and `zeros(<int>)`; `nn.relu` is wrapped to record how close a pre-activation comes
to the kink.

The maker drives `sess.run((model.loss, model.optimizer), feed_dict)` itself on padded feeds built by FISM's rule
(make_golden_fism.feed_of / pad: positive = the history without the item, negative = the whole history, num_idx =
|H| + 1, histories padded with num_items to the longest of their side) — so every instance shorter than the longest
carries the reference's padding term.  predict() is the reference's.

    python tests/golden/make_golden_nais.py              # needs the reference tree

Writes tests/golden/tfgraph_nais.npz and, for the case `a0_none_ce` alone (its 1,100-item history moves 1,100 rows of
c1: one file would pass the size limit of a committed fixture), tests/golden/tfgraph_nais_long.npz:
  indptr / indices / shape     make_golden_fism.train_matrix()
  c1_0 / Q0 / bias_0 / W0_a0 / W0_a1 / b_0 / h_0     the initial tables (W per algorithm)
  cases, <case>_hyper          the case names and, per case, (algorithm, activation or -1, alpha, beta) ; the loss,
                               learner and pairwise flag are in tests/test_nais_cpu.py's CASES
  <case>_users/_items/_third   the batches [steps, B]
  <case>_rows_{c1,Q,bias}, <case>_{f32,f64}_{c1,Q,bias}      as tfgraph_fism.npz: moved rows, float64 differences
  <case>_{f32,f64}_{W,b,h}     [steps, ...] float64 differences from the initial value; <case>_{f32,f64}_loss [steps]
  predict_users, predict_a{0,1}_{f32,f64}      predict() rows after the last step of the cases `a0_none_ce` / `a1_tanh`
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_models as rm          # noqa: E402
from oracle import tf_shim                    # noqa: E402
from make_golden_tfgraph import WIDTHS, _np, _reset_recorders   # noqa: E402
import make_golden_fism as MF                 # noqa: E402

D, WSIZE = 16, 16
# the shipped key set (conf/NAIS.properties) with the test's sizes; activation "Relu" matches none of 0 / 1 / 2
HYPER = dict(pretrain=1, verbose=1, learner="adam", batch_size=64, epochs=1, weight_size=WSIZE, embedding_size=D,
             data_alpha=0, regs=[0.01, 0.02, 1e-5], alpha=0, beta=0.5, num_neg=4, learning_rate=0.01,
             activation="Relu", algorithm=0, is_pairwise=False, loss_function="cross_entropy", topk=20,
             embed_init_method="tnormal", weight_init_method="he_normal", stddev=0.01, pretrain_file="None")
# case -> (hyper overrides, steps, steps in which the 1,100-item user takes part)
CASES = {
    "a0_none_ce": (dict(), 2, (1,)),
    "a0_relu_square": (dict(activation=0, loss_function="square", alpha=0.5), 2, ()),
    "a1_tanh": (dict(algorithm=1, activation=2, loss_function="square", alpha=0.5), 2, ()),
    "a0_sigmoid_b1": (dict(activation=1, beta=1.0, loss_function="square"), 2, ()),
    "gd": (dict(learner="gd", loss_function="square"), 2, ()),
    "adagrad": (dict(learner="adagrad", loss_function="square"), 2, ()),
    "rmsprop": (dict(learner="rmsprop", loss_function="square"), 2, ()),
    "momentum": (dict(learner="momentum", loss_function="square"), 2, ()),
    "bpr": (dict(loss_function="bpr", is_pairwise=True, alpha=0.5), 2, ()),
}
KINK = {"min": np.inf}


# ------------------------------------------------------------------ the call forms NAIS needs on top of the shim
def _ints(vals):
    return [int(v) for v in vals]


def _reshape(x, shape, name=None):
    return tf_shim.Tensor(lambda a, *s: a.reshape(_ints(s)), [x] + list(shape))


def _stack(values, axis=0, name=None):
    def f(*xs):
        if all(isinstance(v, torch.Tensor) for v in xs):
            return torch.stack(xs, dim=axis)
        return tuple(int(v) for v in xs)                       # a shape made of python ints and shape entries
    return tf_shim.Tensor(f, list(values))


def _tile(x, multiples, name=None):
    return tf_shim.Tensor(lambda a, m: a.repeat(*_ints(m)), [x, multiples])


def _sequence_mask(lengths, maxlen=None, dtype=None, name=None):
    """array_ops.sequence_mask: row k is 1 at the positions < lengths[k], of maxlen columns"""
    return tf_shim.Tensor(lambda l, n: (torch.arange(int(n))[None, :] < l[:, None]).to(tf_shim.float_dtype()),
                          [lengths, maxlen])


def _ones(shape, dtype=None, name=None):
    return tf_shim.Tensor(lambda: torch.ones(*_ints(shape), dtype=tf_shim.float_dtype()), [])


def _relu(x, name=None):
    def f(a):
        if a.dtype == torch.float64 and a.numel():
            KINK["min"] = min(KINK["min"], float(a.detach().abs().min()))
        return torch.relu(a)
    return tf_shim.Tensor(f, [x])


def attach_ops():
    MF.attach_ops()
    tf_shim.reshape, tf_shim.stack, tf_shim.tile = _reshape, _stack, _tile
    tf_shim.sequence_mask, tf_shim.ones = _sequence_mask, _ones
    tf_shim.nn.relu = _relu


# ------------------------------------------------------------------ the runs
def run_case(R, init, hyper, batches, predict_users=None):
    out, I = {}, R.shape[1]
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess, _ = rm.build("NAIS", rm.Dataset(R), hyper, width)
        assert any("load pretrained params unsuccessful!" in ln for ln in rm.MemoryLogger.lines)
        model.c1.load(init["c1"])
        model.embedding_Q.load(init["Q"])
        model.bias.load(init["bias"])
        model.W.load(init["W_a%d" % hyper["algorithm"]])
        model.b.load(init["b"].reshape(1, -1))
        model.h.load(init["h"].reshape(-1, 1))
        tabs, losses = [], []
        for users, items, third in batches:
            if hyper["is_pairwise"]:
                hp, np_ = MF.feed_of(R, users, items, [1] * len(users))
                hn, nn = MF.feed_of(R, users, third, [0] * len(users))
                feed = {model.user_input: MF.pad(hp, I), model.user_input_neg: MF.pad(hn, I), model.num_idx: np_,
                        model.num_idx_neg: nn, model.item_input: items, model.item_input_neg: third}
            else:
                h, n = MF.feed_of(R, users, items, third > 0.5)
                feed = {model.user_input: MF.pad(h, I), model.num_idx: n, model.item_input: items, model.labels: third}
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=feed)
            losses.append(float(loss))
            tabs.append((model.c1.numpy(), model.embedding_Q.numpy(), model.bias.numpy(), model.W.numpy(),
                         model.b.numpy().reshape(-1), model.h.numpy().reshape(-1)))
        out[tag] = (tabs, np.asarray(losses, np.float64))
        if predict_users is not None:
            out[tag + "_predict"] = _np(np.stack(model.predict(list(predict_users), None)), width)
    return out


def pack(case, res, init, batches):
    out = MF.pack(case, {t: ([tb[:3] for tb in res[t][0]], res[t][1]) for t, _ in WIDTHS}, init["c1"], init["Q"],
                  init["bias"], batches)
    alg = init["alg"]
    for j, name in ((3, "W"), (4, "b"), (5, "h")):
        base = init["W_a%d" % alg if name == "W" else name].astype(np.float64)
        for tag, _ in WIDTHS:
            out["%s_%s_%s" % (case, tag, name)] = np.stack([t[j].astype(np.float64) - base for t in res[tag][0]])
    return out


def initial_tables(I):
    rs = np.random.RandomState(1811)
    f = lambda x: x.astype(np.float32)
    sign = np.where(rs.rand(WSIZE) < 0.5, -1.0, 1.0)
    return dict(c1=f(0.2 * rs.randn(I, D)), Q=f(0.2 * rs.randn(I, D)), bias=f(0.01 * rs.randn(I)),
                W_a0=f(0.3 * rs.randn(D, WSIZE)), W_a1=f(0.3 * rs.randn(2 * D, WSIZE)),
                b=f(sign * (0.3 + 0.2 * rs.rand(WSIZE))),       # away from zero, both sides of the kink
                h=f(1.0 + 0.3 * rs.randn(WSIZE)))                # not all ones


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_ops()
    MF.register_util_modules()
    R = MF.train_matrix()
    U, I = R.shape
    init = initial_tables(I)
    deg = np.diff(R.indptr)
    one = int(np.flatnonzero(deg == 1)[0])
    hubby = int(np.argmax(deg[:U - 3]))
    some = [int(u) for u in np.flatnonzero(deg[:U - 3] > 2) if u not in (one, hubby)][3]
    predict_users = np.asarray([one, hubby, some, U - 2, U - 1], np.int32)
    out = dict(indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32), shape=np.asarray(R.shape, np.int64),
               c1_0=init["c1"], Q0=init["Q"], bias_0=init["bias"], W0_a0=init["W_a0"], W0_a1=init["W_a1"],
               b_0=init["b"], h_0=init["h"], predict_users=predict_users,
               regs=np.asarray(HYPER["regs"], np.float64), learning_rate=np.float64(HYPER["learning_rate"]),
               cases=np.asarray(sorted(CASES)))
    for k, (case, (over, steps, big_steps)) in enumerate(sorted(CASES.items())):
        hyper = dict(HYPER, **over)
        batches = MF.make_batches(R, steps, big_steps, hyper["is_pairwise"], seed=300 + k)
        KINK["min"] = np.inf
        want_predict = case in ("a0_none_ce", "a1_tanh")
        res = run_case(R, init, hyper, batches, predict_users if want_predict else None)
        if hyper["activation"] == 0:
            # no pre-activation of the f64 run near the kink: no f32 rounding can flip a relu
            assert 1e-4 < KINK["min"] < np.inf, KINK
        out.update(pack(case, res, dict(init, alg=hyper["algorithm"]), batches))
        act = hyper["activation"] if hyper["activation"] in (0, 1, 2) else -1
        out[case + "_hyper"] = np.asarray([hyper["algorithm"], act, hyper["alpha"], hyper["beta"]], np.float64)
        if want_predict:
            a = hyper["algorithm"]
            out["predict_a%d_f32" % a] = res["f32_predict"].astype(np.float32)
            out["predict_a%d_f64" % a] = res["f64_predict"]
        print(case, "losses", res["f64"][1], "kink", KINK["min"])
    long_keys = [k for k in out if k.startswith("a0_none_ce_")]
    for name, part in (("tfgraph_nais.npz", {k: v for k, v in out.items() if k not in long_keys}),
                       ("tfgraph_nais_long.npz", {k: out[k] for k in long_keys})):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
