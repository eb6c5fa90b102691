"""Golden DeepICF trace produced by the REFERENCE's own class (model/general_recommender/DeepICF.py).

The class is loaded whole and unchanged (make_golden_neumf.load_class) and run under oracle/tf_shim.py, in float32 and
float64.  The ops the shim lacks are attached HERE, by their published definitions [EXT: tensorflow r1.12], and each is
put on a hand-computed value first (check_ops): the call forms NAIS needs (make_golden_nais.attach_ops: sequence_mask,
tile, stack, reshape on shape entries, ones, constant(value, dtype, shape), zeros(<int>)), `cond`,
`losses.log_loss` and the contrib `batch_norm`, reachable as `tensorflow.contrib.layers.python.layers.batch_norm`.
pow, div and add_n are the shim's own.  Nothing under oracle/ changes.

The batch norm adopted [EXT: tensorflow r1.12, contrib/layers/python/layers/layers.py `batch_norm` and
`_fused_batch_norm`; core/kernels/fused_batch_norm_op.cc `FusedBatchNorm<CPUDevice>`; python/training/
moving_averages.py `assign_moving_average`]: batch_norm(decay=0.9, center=True, scale=True, epsilon=0.001,
updates_collections=None, fused=None) on a rank-2 input takes the fused path.  Per scope it creates beta (zeros,
trainable), gamma (ones, trainable), moving_mean (zeros) and moving_variance (ones), both not trainable.
  is_training=True:   y = gamma (x - mean) / sqrt(var + epsilon) + beta with the batch mean and the BIASED batch
                      variance over the N rows; then, in place (updates_collections=None),
                      moving_mean -= (moving_mean - mean) (1 - decay) and
                      moving_variance -= (moving_variance - var N / max(N - 1, 1)) (1 - decay):
                      the kernel hands the UNBIASED variance to the moving average and normalises with the biased one
  is_training=False:  y = gamma (x - moving_mean) / sqrt(moving_variance + epsilon) + beta
The class builds BOTH forms per layer outside tf.cond, so a real TF-1.12 predict() also runs the training form and
moves the statistics, in an order relative to the inference form's read that the graph leaves open.  That is NOT
reproduced: here the in-place update is committed by the `cond` only when its predicate is true, so predict() reads
the moving statistics and changes nothing.

    python tests/golden/make_golden_deepicf.py              # needs the reference tree

Writes tests/golden/tfgraph_deepicf.npz and, for the cases `adagrad`, `rmsprop` and `epoch` (one file would pass the
size limit of a committed fixture), tests/golden/tfgraph_deepicf_more.npz:
  shape, indptr, indices         make_golden_tfgraph.toy_matrix(): 157 x 131, users without train items among them
  cases; <case>_hyper_json       the case names and their hyper-parameters; the initial variables of a case are
                                 deepicf_restatement.init_tables(131, d, w, layers, algorithm, batch_norm, <case>_init_seed)
  <case>_steps; <case>_{users,items,labels}_<s>   the fed instances of step s.  Every 6-instance step holds a repeated
                                 (user, item), an item that is a target and in another instance's history, and a user
                                 with ONE train item as a positive (it pools nothing but the padding row)
  <case>_loss_{f32,f64} [S]      the loss of each step (before its update)
  <case>_f64_<var> [S, ...]      every variable (moving statistics included) after each step of the float64 run MINUS
                                 its initial value;  <case>_gap_<var> [S]: max |float32 run - float64 run|
  forms_json                     {variable: "rows" | "dense"}: the optimiser form the stand-in's trace took per variable
  predict_users [27], predict_cand [27, 3], predict_<case>_{f32,f64} [27, 131], predict_<case>_cand_{f32,f64} [27, 3]
                                 predict() after the last step of `default`, full and candidate mode
  epoch_*                        one train_model() epoch of `default` at batch_size 16 and the shipped learning_rate
                                 0.001 under numpy seed epoch_seed on
                                 toy_matrix(isolated=False) (train_model reads train_dict[u] of EVERY user): the fed
                                 (users, items, labels) of every step — the last is partial —, the losses, the end
                                 variables under the case name `epoch`, and predict() after it (predict_epoch_*)
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_models as rm          # noqa: E402
from oracle import tf_shim                    # noqa: E402
from make_golden_tfgraph import WIDTHS, _np, _reset_recorders, toy_matrix   # noqa: E402
import make_golden_neumf as N                 # noqa: E402
import make_golden_nais as MN                 # noqa: E402
import deepicf_restatement as R               # noqa: E402

B_STEP, B_EPOCH, STEPS, N_PREDICT = 6, 16, 3, 27
EPOCH_SEED, EPOCH_INIT_SEED = 4127, 1990
BN_PATH = ("tensorflow.contrib.layers.python", "tensorflow.contrib.layers.python.layers")

# the shipped key set (conf/DeepICF.properties); learning_rate 0.01 so that three steps move the tables visibly
HYPER = dict(pretrain_file="None", verbose=1, learner="adam", batch_size=256, epochs=1, layers=[64, 32, 16],
             weight_size=16, embedding_size=16, data_alpha=0, regs=[0.000001, 0.000001, 0.00001], regw=[10, 10],
             alpha=0, beta=0.5, num_neg=4, learning_rate=0.01, activation="Relu", algorithm=1, batch_norm=1,
             embed_init_method="tnormal", weight_init_method="he_normal", bias_init_method="he_normal", stddev=0.01)
BIG_REGS = [0.01, 0.02, 0.001]
CASES = {
    "default": dict(),
    "prod_nobn": dict(algorithm=0, activation=0, batch_norm=0, layers=[8], regw=[], alpha=0.5, beta=1.0, regs=BIG_REGS),
    "odd": dict(embedding_size=7, weight_size=5, layers=[12, 5], activation=2, batch_norm=1, regw=[10, 0, 10],
                alpha=0.25, regs=BIG_REGS),
    "adagrad": dict(learner="adagrad", regs=BIG_REGS),
    "rmsprop": dict(learner="rmsprop", regs=BIG_REGS),
    "saturated": dict(algorithm=0, activation=0, batch_norm=0, layers=[8], regw=[], alpha=0.5, beta=1.0, regs=BIG_REGS,
                      bias_scale=200.0),     # outputs near 0 and 1: the 1e-7 inside the loss's logarithms matters
    "single": dict(),                         # steps of ONE instance: zero batch variance, the max(N - 1, 1) guard
}
MORE = ("adagrad", "rmsprop", "epoch")       # the cases kept in tfgraph_deepicf_more.npz: one file would pass 1 MiB
PENDING = []                                  # moving-statistics updates a training batch norm has computed
KINK = MN.KINK


# ------------------------------------------------------------------ the ops the shim lacks
def _batch_norm(inputs, decay=0.999, center=True, scale=False, epsilon=0.001, updates_collections=None,
                is_training=True, reuse=None, trainable=True, scope=None, **_):
    assert center and scale and updates_collections is None
    scopes = tf_shim._GRAPH.__dict__.setdefault("bn_scopes", {})
    if reuse:
        beta, gamma, mm, mv = scopes[scope]
    else:
        n = int(inputs.static_width)
        beta = tf_shim.Variable(np.zeros(n, np.float32), name="%s/beta" % scope, trainable=trainable)
        gamma = tf_shim.Variable(np.ones(n, np.float32), name="%s/gamma" % scope, trainable=trainable)
        mm = tf_shim.Variable(np.zeros(n, np.float32), name="%s/moving_mean" % scope, trainable=False)
        mv = tf_shim.Variable(np.ones(n, np.float32), name="%s/moving_variance" % scope, trainable=False)
        scopes[scope] = (beta, gamma, mm, mv)

    def train(x, b, g, m, v):
        n_rows = x.shape[0]
        mean = x.mean(dim=0)
        var = ((x - mean[None, :]) ** 2).mean(dim=0)
        with torch.no_grad():
            unbiased = var * (n_rows / max(n_rows - 1, 1))
            PENDING.append((mm, m - (m - mean) * (1 - decay), mv, v - (v - unbiased) * (1 - decay)))
        return g[None, :] * ((x - mean[None, :]) / torch.sqrt(var + epsilon)[None, :]) + b[None, :]

    def infer(x, b, g, m, v):
        return g[None, :] * ((x - m[None, :]) / torch.sqrt(v + epsilon)[None, :]) + b[None, :]
    return tf_shim.Tensor(train if is_training else infer, [inputs, beta, gamma, mm, mv])


def _cond(pred, true_fn=None, false_fn=None, name=None, **_):
    """control_flow_ops.cond on tensors built outside it: the value of the taken branch.  The training batch norm's
    in-place update is committed here, when the predicate is true (the module's docstring has why)"""
    def f(p, a, b):
        if bool(p):
            for mm, new_m, mv, new_v in PENDING:
                mm.value, mv.value = new_m.detach().clone(), new_v.detach().clone()
        del PENDING[:]
        return a if bool(p) else b
    return tf_shim.Tensor(f, [pred, true_fn(), false_fn()])


def _log_loss(labels, predictions, weights=1.0, epsilon=1e-7, **_):
    """losses_impl.log_loss: -y log(p + eps) - (1 - y) log(1 - p + eps), reduced by SUM_BY_NONZERO_WEIGHTS: the MEAN"""
    return tf_shim.Tensor(lambda y, p: (-y * torch.log(p + epsilon) - (1 - y) * torch.log(1 - p + epsilon)).mean(),
                          [labels, predictions])


def _matmul(a, b, **k):
    """the shim's matmul, with the static width of its result kept for batch_norm's variable shapes"""
    out = SHIM_MATMUL(a, b, **k)
    if isinstance(b, tf_shim.Variable):
        out.static_width = int(b.value.shape[1])
    return out


def _add(a, b, name=None):
    out = SHIM_ADD(a, b)
    if hasattr(a, "static_width"):
        out.static_width = a.static_width
    return out


SHIM_MATMUL, SHIM_ADD = tf_shim.matmul, tf_shim.add


def attach_ops():
    MN.attach_ops()
    if tf_shim.matmul is not _matmul:
        tf_shim.matmul, tf_shim.add = _matmul, _add
    tf_shim.cond = _cond
    tf_shim.losses.log_loss = _log_loss
    py = types.ModuleType(BN_PATH[0])
    py.__path__ = []
    layers = types.ModuleType(BN_PATH[1])
    layers.batch_norm = _batch_norm
    py.layers = layers
    return {BN_PATH[0]: py, BN_PATH[1]: layers}


def check_ops():
    """every op attached here on a small hand-computed value"""
    tf = tf_shim
    tf.set_float("float64")
    tf.reset_default_graph()
    tf._GRAPH.__dict__.pop("bn_scopes", None)
    sess = tf.Session(seed=0)
    y = tf.constant(np.asarray([1.0, 0.0]))
    p = tf.constant(np.asarray([0.5, 0.25]))
    want = (-np.log(0.5 + 1e-7) - np.log(0.75 + 1e-7)) / 2
    assert abs(float(sess.run(tf.losses.log_loss(y, p))) - want) < 1e-15
    assert sess.run(tf.sequence_mask(tf.constant(np.asarray([1.0, 3.0])), maxlen=2, dtype=tf.float32)).tolist() == \
        [[1.0, 0.0], [1.0, 1.0]]
    assert sess.run(tf.pow(tf.constant(np.asarray([4.0])), tf.constant(0.5, tf.float32, [1]))).tolist() == [2.0]
    assert sess.run(tf.div(tf.constant(np.asarray([3.0])), tf.constant(np.asarray([4.0])))).tolist() == [0.75]
    assert sess.run(tf.add_n([tf.constant(np.asarray([1.0])), tf.constant(np.asarray([2.5]))])).tolist() == [3.5]
    assert sess.run(tf.tile(tf.constant(np.asarray([[[1.0, 2.0]]])), tf.stack([1, 2, 1]))).tolist() == \
        [[[1.0, 2.0], [1.0, 2.0]]]
    # batch norm on x = [[1, 10], [3, 10], [8, 10]]: mean [4, 10], biased variance [26/3, 0], unbiased [13, 0]
    x = tf.placeholder(tf.float32, [None, 2])
    w = tf.Variable(np.eye(2))
    phase = tf.placeholder(tf.bool)
    z = tf.matmul(x, w)
    a = _batch_norm(z, decay=0.9, center=True, scale=True, updates_collections=None, is_training=True, reuse=None,
                    scope="t")
    b = _batch_norm(z, decay=0.9, center=True, scale=True, updates_collections=None, is_training=False, reuse=True,
                    scope="t")
    out = tf.cond(phase, lambda: a, lambda: b)
    beta, gamma, mm, mv = tf._GRAPH.bn_scopes["t"]
    assert [v.trainable for v in (beta, gamma, mm, mv)] == [True, True, False, False]
    gamma.load(np.asarray([2.0, 1.0]))
    beta.load(np.asarray([0.5, -1.0]))
    xs = np.asarray([[1.0, 10.0], [3.0, 10.0], [8.0, 10.0]])
    got = sess.run(out, feed_dict={x: xs, phase: False})           # moving statistics 0 / 1, nothing moves
    assert np.allclose(got, np.asarray([2.0, 1.0]) * xs / np.sqrt(1.001) + np.asarray([0.5, -1.0]), atol=1e-14)
    assert mm.numpy().tolist() == [0.0, 0.0] and mv.numpy().tolist() == [1.0, 1.0]
    got = sess.run(out, feed_dict={x: xs, phase: True})
    sd = np.sqrt(26.0 / 3.0 + 0.001)
    assert np.allclose(got[:, 0], 2.0 * np.asarray([-3.0, -1.0, 4.0]) / sd + 0.5, atol=1e-14)
    assert np.allclose(got[:, 1], -1.0, atol=1e-14)                 # zero variance: beta alone
    assert np.allclose(mm.numpy(), [0.4, 1.0], atol=1e-12) and np.allclose(mv.numpy(), [0.9 + 1.3, 0.9], atol=1e-12)
    sess.run(out, feed_dict={x: xs[:1], phase: True})               # one row: variance 0, the max(N - 1, 1) guard
    assert np.allclose(mm.numpy(), [0.36 + 0.1, 0.9 + 1.0], atol=1e-12)
    assert np.allclose(mv.numpy(), [0.9 * 2.2, 0.81], atol=1e-12)
    tf._GRAPH.__dict__.pop("bn_scopes", None)
    tf.reset_default_graph()
    return True


# ------------------------------------------------------------------ the class
VAR_OF = {"c1": "c1", "embedding_Q": "Q", "bias": "bias", "Weights_for_MLP": "W", "Bias_for_MLP": "b",
          "H_for_MLP": "h", "weights_out": "Wout", "biases_out": "bout"}


def _short(name):
    if name in VAR_OF:
        return VAR_OF[name]
    for a, b in (("weights_h", "W"), ("biases_b", "b")):
        if name.startswith(a):
            return b + name[len(a):]
    scope, what = name.split("/")
    return {"beta": "beta", "gamma": "gamma", "moving_mean": "mm", "moving_variance": "mv"}[what] + scope[3:]


def build(ds, hyper, width, extra=None):
    """(model, session, {short name: Variable}, the class's module)"""
    mods = attach_ops()
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    tf_shim._GRAPH.collections = {}
    tf_shim._GRAPH.__dict__.pop("bn_scopes", None)
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        mod = N.load_class("DeepICF")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "DeepICF"
    conf.update(hyper)
    sess = tf_shim.Session(seed=0)
    model = mod.DeepICF(sess, ds, conf)
    prev = tf_shim._RUN["session"]
    tf_shim._RUN["session"] = sess            # biases are Variables of tf.random_normal: drawn while the graph is built
    try:
        model.build_graph()
    finally:
        tf_shim._RUN["session"] = prev
    assert any("load pretrained params unsuccessful!" in ln for ln in rm.MemoryLogger.lines)
    sess.run(tf_shim.global_variables_initializer())
    variables = {_short(v.name): v for v in tf_shim._GRAPH.variables}
    L, bn = len(hyper["layers"]), bool(hyper["batch_norm"])
    assert sorted(variables) == sorted(R.names(L, bn) + R.moving_names(L, bn)), sorted(variables)
    # biases['b%d'] and biases['out'] start from random_normal with stddev 1
    draws = [a for kind, a in sess.draw_log if kind == "random_normal"]
    assert [a.shape for a in draws] == [(1,)] + [(n,) for n in hyper["layers"]]
    return model, sess, variables, mod


def load_tables(variables, init):
    for k, v in variables.items():
        v.load(init[k].reshape(tuple(v.value.shape)))


def init_of(hyper, I, seed):
    return R.init_tables(I, hyper["embedding_size"], hyper["weight_size"], hyper["layers"], hyper["algorithm"],
                         bool(hyper["batch_norm"]), seed, hyper.get("bias_scale", 1.0))


def restated_hyper(hyper):
    """the hyper-parameters in the restatement's (and the engine's) terms"""
    act = hyper["activation"]
    return dict(algorithm=hyper["algorithm"], activation=act if act in (0, 1, 2) else -1, alpha=float(hyper["alpha"]),
                beta=float(hyper["beta"]), layers=list(hyper["layers"]), batch_norm=int(bool(hyper["batch_norm"])),
                regs=[float(x) for x in hyper["regs"]], regw=[float(x) for x in hyper["regw"]],
                d=hyper["embedding_size"], w=hyper["weight_size"], learner=hyper["learner"],
                lr=float(hyper["learning_rate"]), bias_scale=float(hyper.get("bias_scale", 1.0)))


def feed_of(model, mod, Rm, users, items, labels):
    """the feed train_model builds (DeepICF.py:213-219) for instances by data_generator.py:29-54"""
    hist, num = [], []
    for u, i, y in zip(users, items, labels):
        its = Rm.indices[Rm.indptr[u]:Rm.indptr[u + 1]].tolist()
        if y > 0.5:
            its.remove(int(i))
        num.append(len(its) + 1)                                    # positive: size; negative: size + 1
        hist.append(its)
    return {model.user_input: mod.pad_sequences(hist, value=Rm.shape[1]), model.num_idx: np.asarray(num, np.float32),
            model.item_input: np.asarray(items, np.int32), model.labels: np.asarray(labels, np.float32),
            model.is_train_phase: True}


def make_batches(Rm, steps, seed, single=False):
    rs = np.random.RandomState(seed)
    deg = np.diff(Rm.indptr)
    row = lambda u: Rm.indices[Rm.indptr[u]:Rm.indptr[u + 1]]
    ones = np.flatnonzero(deg == 1)
    many = np.flatnonzero(deg > 2)
    assert len(ones) and len(many) > 8

    def neg(u, among=None):
        pool = np.setdiff1d(np.arange(Rm.shape[1]) if among is None else among, row(u))
        return int(pool[rs.randint(len(pool))])
    out = []
    for s in range(steps):
        while True:
            ua, ub, uc, ud = (int(u) for u in rs.choice(many, 4, replace=False))
            ia = int(row(ua)[rs.randint(deg[ua])])
            others = np.setdiff1d(np.setdiff1d(row(ua), [ia]), row(ub))
            if len(others):
                break
        one = int(ones[s % len(ones)])
        inst = [(ua, ia, 1.0), (ua, ia, 1.0),                       # a repeated (user, item)
                (ub, neg(ub, others), 0.0),                         # a target that is in ua's pooled history
                (one, int(row(one)[0]), 1.0),                       # pools nothing but the padding row
                (uc, int(row(uc)[rs.randint(deg[uc])]), 1.0), (ud, neg(ud), 0.0)]
        if single:
            inst = [inst[(0, 3, 5)[s % 3]]]
        else:
            inst = [inst[j] for j in rs.permutation(len(inst))]
        out.append((np.asarray([x[0] for x in inst], np.int32), np.asarray([x[1] for x in inst], np.int32),
                    np.asarray([x[2] for x in inst], np.float32)))
    return out


def run_case(ds, hyper, init, batches, predict=None):
    Rm, out = ds.train_matrix, {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess, variables, mod = build(ds, hyper, width)
        load_tables(variables, init)
        tabs, losses = [], []
        for users, items, labels in batches:
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=feed_of(model, mod, Rm, users, items, labels))
            losses.append(float(loss))
            tabs.append({k: v.numpy().reshape(init[k].shape) for k, v in variables.items()})
        out[tag] = (tabs, losses)
        out["forms"] = {k: ("rows" if model.optimizer.sparse[id(v)] else "dense") for k, v in variables.items()
                        if id(v) in model.optimizer.sparse}
        out["kink"] = KINK["min"]                                   # of the training steps: predict() is continuous
        if predict is not None:
            out[tag + "_predict"] = run_predict(model, variables, predict, width)
    return out


def run_predict(model, variables, predict, width):
    users, cand = predict
    before = {k: v.numpy() for k, v in variables.items()}
    full = _np(np.stack(model.predict(list(users), None)), width)
    some = _np(np.stack(model.predict(list(users), [list(c) for c in cand])), width)
    assert all(np.array_equal(before[k], v.numpy()) for k, v in variables.items())     # predict() moves nothing
    return full, some


def pack_tables(case, tabs_by_tag, init):
    out = {}
    for name in tabs_by_tag["f64"][0]:
        want = np.stack([t[name] for t in tabs_by_tag["f64"]]).astype(np.float64)
        twin = np.stack([t[name] for t in tabs_by_tag["f32"]]).astype(np.float64)
        out["%s_f64_%s" % (case, name)] = want - init[name].astype(np.float64)[None]
        out["%s_gap_%s" % (case, name)] = np.abs(twin - want).reshape(len(want), -1).max(axis=1, initial=0)
    return out


class Hist(list):
    """a history list that remembers its user (the feeds hold histories, the device takes users)"""
    user = -1


def run_epoch(ds, hyper, init, predict):
    """one whole train_model(): the class draws its own negatives and shuffles (numpy's stream, seeded); the users of
    the fed histories are read off the lists the generator made"""
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        rm.RecordingEvaluator.users = [0]
        model, sess, variables, mod = build(ds, hyper, width)
        load_tables(variables, init)
        fed, gen, pad = [], mod.data_generator._get_pointwise_all_likefism_data, mod.pad_sequences

        def generate(dataset, num_negatives, train_dict):
            user_input, num_idx, item_input, labels = gen(dataset, num_negatives, train_dict)
            k, tagged = 0, []
            for u in range(dataset.num_users):
                for _ in range(len(train_dict[u]) * (num_negatives + 1)):
                    h = Hist(user_input[k])
                    h.user = u
                    tagged.append(h)
                    k += 1
            assert k == len(user_input)
            return tagged, num_idx, item_input, labels

        def pad_and_log(sequences, **kw):
            if all(isinstance(s, Hist) for s in sequences):
                fed.append([s.user for s in sequences])
            return pad(sequences, **kw)

        losses, feeds = [], []
        run = sess.run

        def logged_run(fetches, feed_dict=None):
            res = run(fetches, feed_dict=feed_dict)
            if isinstance(fetches, tuple) and feed_dict is not None and model.labels in feed_dict:
                losses.append(float(res[0]))
                feeds.append((np.asarray(feed_dict[model.item_input], np.int32),
                              np.asarray(feed_dict[model.labels], np.float32),
                              np.asarray(feed_dict[model.num_idx], np.float32)))
            return res
        sess.run = logged_run
        mod.data_generator._get_pointwise_all_likefism_data, mod.pad_sequences = generate, pad_and_log
        np.random.seed(EPOCH_SEED)
        try:
            model.train_model()
        finally:
            mod.data_generator._get_pointwise_all_likefism_data, mod.pad_sequences = gen, pad
        sess.run = run
        assert len(fed) == len(feeds) and any("[iter 1 : loss : " in ln for ln in rm.MemoryLogger.lines)
        deg = np.diff(ds.train_matrix.indptr)
        for users, (items, labels, num) in zip(fed, feeds):           # num_idx: size (positive), size + 1 (negative)
            assert np.array_equal(num, deg[users] + (labels < 0.5))
        out[tag] = dict(users=[np.asarray(u, np.int32) for u in fed], items=[f[0] for f in feeds],
                        labels=[f[1] for f in feeds], losses=losses,
                        tabs=[{k: v.numpy().reshape(init[k].shape) for k, v in variables.items()}],
                        lines=list(rm.MemoryLogger.lines), predict=run_predict(model, variables, predict, width))
    a, b = out["f32"], out["f64"]
    assert len(a["users"]) == len(b["users"])
    for k in ("users", "items", "labels"):
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_ops()
    check_ops()
    Rm = toy_matrix(isolated=True)
    U, I = Rm.shape
    ds = rm.Dataset(Rm)
    out = dict(shape=np.asarray(Rm.shape, np.int64), indptr=Rm.indptr.astype(np.int64),
               indices=Rm.indices.astype(np.int32), cases=np.asarray(sorted(CASES)))
    rs = np.random.RandomState(11)
    deg = np.diff(Rm.indptr)
    predict_users = np.sort(rs.choice(np.flatnonzero(deg > 0), N_PREDICT, replace=False)).astype(np.int32)
    cand = rs.randint(0, I, (N_PREDICT, 3)).astype(np.int32)
    out.update(predict_users=predict_users, predict_cand=cand)
    gaps, forms = {}, None
    for k, case in enumerate(sorted(CASES)):
        hyper = dict(HYPER, **CASES[case])
        init = init_of(hyper, I, 1300 + k)
        batches = make_batches(Rm, STEPS, 5200 + k, single=case == "single")
        KINK["min"] = np.inf
        res = run_case(ds, hyper, init, batches, (predict_users, cand) if case == "default" else None)
        assert res["kink"] > 1e-5, (case, res["kink"])              # no f32 rounding flips a relu of the f64 steps
        assert forms is None or all(forms[n] == f for n, f in res["forms"].items() if n in forms)
        forms = dict(forms or {}, **res["forms"])
        out["%s_hyper_json" % case] = np.asarray(json.dumps(restated_hyper(hyper)))
        out["%s_init_seed" % case] = np.int64(1300 + k)
        out["%s_steps" % case] = np.int64(len(batches))
        for s, (users, items, labels) in enumerate(batches):
            out["%s_users_%d" % (case, s)], out["%s_items_%d" % (case, s)] = users, items
            out["%s_labels_%d" % (case, s)] = labels
        for tag, _ in WIDTHS:
            out["%s_loss_%s" % (case, tag)] = np.asarray(res[tag][1], np.float64)
            if case == "default":
                out["predict_%s_%s" % (case, tag)], out["predict_%s_cand_%s" % (case, tag)] = res[tag + "_predict"]
        out.update(pack_tables(case, {tag: res[tag][0] for tag, _ in WIDTHS}, init))
        gaps[case] = max(out["%s_gap_%s" % (case, n)].max(initial=0) for n in res["f64"][0][0])
        print(case, "losses", res["f64"][1], "kink", res["kink"], "gap %.3g" % gaps[case])
    out["forms_json"] = np.asarray(json.dumps(forms))
    # the epoch
    Re = toy_matrix(isolated=False)
    hyper = dict(HYPER, batch_size=B_EPOCH, learning_rate=0.001)    # the shipped rate: the unbounded exp() of the
    init = init_of(hyper, I, EPOCH_INIT_SEED)                       # attention leaves the float range at 0.01
    KINK["min"] = np.inf
    ep = run_epoch(rm.Dataset(Re), hyper, init, (predict_users, cand))
    e64 = ep["f64"]
    sizes = np.asarray([len(u) for u in e64["users"]], np.int64)
    assert sizes[-1] < B_EPOCH and (sizes[:-1] == B_EPOCH).all()    # the last batch is partial
    out.update(epoch_indptr=Re.indptr.astype(np.int64), epoch_indices=Re.indices.astype(np.int32),
               epoch_sizes=sizes, epoch_users=np.concatenate(e64["users"]), epoch_items=np.concatenate(e64["items"]),
               epoch_labels=np.concatenate(e64["labels"]), epoch_seed=np.int64(EPOCH_SEED),
               epoch_init_seed=np.int64(EPOCH_INIT_SEED), epoch_hyper_json=np.asarray(json.dumps(restated_hyper(hyper))),
               epoch_log=np.asarray([ln for ln in e64["lines"] if ln.startswith(("[iter", "epoch", "load"))]))
    for tag, _ in WIDTHS:
        out["epoch_loss_%s" % tag] = np.asarray(ep[tag]["losses"], np.float64)
        out["predict_epoch_%s" % tag], out["predict_epoch_cand_%s" % tag] = ep[tag]["predict"]
    out.update(pack_tables("epoch", {tag: ep[tag]["tabs"] for tag, _ in WIDTHS}, init))
    gaps["epoch"] = max(out["epoch_gap_%s" % n].max(initial=0) for n in e64["tabs"][0])
    more = [k for k in out if k.split("_")[0] in MORE or k.startswith("predict_epoch")]
    for name, part in (("tfgraph_deepicf.npz", {k: v for k, v in out.items() if k not in more}),
                       ("tfgraph_deepicf_more.npz", {k: out[k] for k in more})):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    print("%d epoch steps, kink %.3g; fp32 vs fp64 gaps %s; forms %s" % (
        len(sizes), KINK["min"], {k: "%.3g" % v for k, v in gaps.items()}, forms))


if __name__ == "__main__":
    main()
