"""Golden SASRec trace produced by the REFERENCE's own SASRec class (model/sequential_recommender/SASRec.py).

The class is loaded whole and unchanged with oracle/ref_models._load_file and runs under oracle/tf_shim.py, as
make_golden_gru4recplus.py loads its class.  Ops of SASRec.py the shim lacks are attached from here (attach_sasrec_ops)
by their published definitions [EXT: tensorflow r1.12], each checked on a small hand-computed value before use.

Stand-ins for the surroundings, as in the other makers: `util.DataIterator`, `pad_sequences` and
`csr_to_user_dict_bytime` are the reference's own files; `batch_randint_choice` (Cython over glibc rand() in the
reference) is sasrec_restatement's numpy-stream sampler.  The reference's sampler raises for a request of size 0 (a user
with one train item) and hands back a bare int for size 1 (a user with two), which `pad_sequences` cannot take; the
stand-in returns a list in both cases so that such users run: an empty list is an all-padded row.

    python tests/golden/make_golden_sasrec.py              # needs the reference tree

Writes tests/golden/tfgraph_sasrec.npz:
  indptr / indices / shape     the train pattern: toy_matrix(isolated=False) (157 x 131)
  seq_ptr / seq                every user's items by time: a seeded permutation of the row (make_golden_fpmc)
  <case>_init_<var>            the initial variables of the case (float32), <var> of sasrec_restatement.table_names
  <case>_seq / _pos / _neg     [steps, B, L] the feeds
  <case>_mask<k>               [steps, ...] uint8: dropout site k of every step, from the session's draw_log (rate > 0)
  <case>_loss_{f32,f64}        [steps] the loss fetched with each step (before its update)
  <case>_rows_item_emb         the rows of item_emb that differ from their initial value at any step, in either width
  <case>_{f32,f64}_<var>       [steps, ...]: those rows (every other variable: whole) after each step MINUS their
                               initial value, stored as float32: the differences are ~1e-3 and lose at most 2^-24 of
                               that, 1e-10, four orders below the tolerance that reads them
  epoch_*                      one train_model() epoch of the case `first` at batch_size 16, rate 0, with a recording
                               session: epoch_seq / _pos / _neg [S, 16, L] (the last batch padded with all-pad rows up
                               to 16, epoch_rows [S] its true size), epoch_seed, the end tables under the case name `epoch`
  predict_users, predict_{f32,f64}, predict_cand, predict_cand_{f32,f64}, user_emb_{f32,f64}
                               predict() after the last step of the case `third`, full and candidate mode, and
                               seq[:, -1, :] of those users
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_models as rm          # noqa: E402
from oracle import tf_shim                    # noqa: E402
from make_golden_tfgraph import WIDTHS, _np, _reset_recorders, toy_matrix   # noqa: E402
from make_golden_fpmc import TimedDataset, time_orders                      # noqa: E402
import make_golden_gru4rec as G               # noqa: E402
import sasrec_restatement as P                # noqa: E402

B_STEP, B_EPOCH, STEPS = 20, 16, 3
EPOCH_SEED = 4244
FEED_SEED = 4245


def load_sasrec():
    """the reference module model/sequential_recommender/SASRec.py, executed under the shim"""
    saved_tf = tf_shim.install()
    shadowed = G._SHADOWED + ("util.data_iterator",)
    saved = {k: sys.modules.get(k) for k in shadowed}
    try:
        tool = rm._load_file("util.tool", os.path.join(rm.REF, "util", "tool.py"))
        it = rm._load_file("util.data_iterator", os.path.join(rm.REF, "util", "data_iterator.py"))
        util = types.ModuleType("util")
        util.__path__ = []
        util.tool, util.data_iterator = tool, it
        for fn in ("timer", "l2_loss", "inner_product", "log_loss", "csr_to_user_dict", "csr_to_user_dict_bytime",
                   "pad_sequences"):
            setattr(util, fn, getattr(tool, fn))
        util.DataIterator = it.DataIterator
        util.batch_randint_choice = P.numpy_batch_randint_choice
        util.Logger = rm.MemoryLogger
        sys.modules["util"] = util
        sys.modules["data"] = types.ModuleType("data")
        ev = types.ModuleType("evaluator")
        ev.ProxyEvaluator = rm.RecordingEvaluator
        sys.modules["evaluator"] = ev
        model_pkg = types.ModuleType("model")
        model_pkg.__path__ = []
        sys.modules["model"] = model_pkg
        rm._load_file("model.AbstractRecommender", os.path.join(rm.REF, "model", "AbstractRecommender.py"))
        mod = rm._load_file("model.sequential_recommender.SASRec",
                            os.path.join(rm.REF, "model", "sequential_recommender", "SASRec.py"))
        sys.modules.pop("model.sequential_recommender.SASRec", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


# ------------------------------------------------------------------ the ops SASRec.py needs beyond the shim's
class _Shape(list):
    def as_list(self):
        return list(self)

    def __getitem__(self, k):
        r = list.__getitem__(self, k)
        return _Shape(r) if isinstance(k, slice) else r


def _static_shape(node):
    """get_shape(): the node evaluated on stand-in feeds (2 rows, flags off) — only fixed dimensions are read from it"""
    import torch
    feeds = {}
    for n in tf_shim._ancestors(node):
        if n.kind == "placeholder" and n.default is None:
            if n.dtype is tf_shim.bool:
                feeds[id(n)] = False
            else:
                feeds[id(n)] = np.zeros([2 if s is None else int(s) for s in (n.shape or [])], np.int64)
    with torch.no_grad():
        return _Shape(int(s) for s in tf_shim._evaluate([node], feeds)[0].shape)


def _dims(parts):
    """a shape / multiples list whose entries may be graph nodes -> (inputs, rebuild)"""
    nodes = [p if isinstance(p, tf_shim.Tensor) else tf_shim._Const(int(p)) for p in parts]
    return nodes


def attach_sasrec_ops():
    import torch
    T = tf_shim.Tensor
    REG = "regularization_losses"
    tf_shim.GraphKeys = types.SimpleNamespace(REGULARIZATION_LOSSES=REG)
    tf_shim.Tensor.get_shape = _static_shape

    def get_collection(key, scope=None):
        return list(getattr(tf_shim._GRAPH, "collections", {}).get(key, []))

    def get_variable(name, shape=None, dtype=None, initializer=None, regularizer=None, trainable=True, **_):
        """variable_scope.get_variable: a new variable (glorot-uniform by default; the makers overwrite it), its
        regulariser's penalty — when it returns one — added to GraphKeys.REGULARIZATION_LOSSES"""
        init = initializer if initializer is not None else tf_shim.contrib.layers.xavier_initializer()
        v = tf_shim.Variable(init([int(s) for s in shape]), trainable=trainable, name=name)
        if regularizer is not None:
            pen = regularizer(v)
            if pen is not None:
                if not hasattr(tf_shim._GRAPH, "collections"):
                    tf_shim._GRAPH.collections = {}
                tf_shim._GRAPH.collections.setdefault(REG, []).append(pen)
        return v

    if not hasattr(tf_shim, "_sasrec_add_n"):
        tf_shim._sasrec_add_n = tf_shim.add_n
    shim_add_n = tf_shim._sasrec_add_n

    def add_n(inputs, name=None):
        """math_ops.add_n: 'inputs must be a list of at least one Tensor' — raised while the graph is built"""
        if not inputs:
            raise ValueError("inputs must be a list of at least one Tensor/IndexedSlices with the same dtype and shape")
        return shim_add_n(inputs)

    def moments(x, axes, shift=None, name=None, keep_dims=False):
        """nn_impl.moments: mean and the BIASED variance mean((x - mean)^2)"""
        ax = tuple(int(a) for a in axes)
        mean = T(lambda a: a.mean(dim=ax, keepdim=bool(keep_dims)), [x])
        var = T(lambda a: ((a - a.mean(dim=ax, keepdim=True)) ** 2).mean(dim=ax, keepdim=bool(keep_dims)), [x])
        return mean, var

    def dense(inputs, units, activation=None, use_bias=True, **_):
        """layers.dense: kernel [in, units] (glorot uniform), then bias [units] (zeros); inputs kernel + bias"""
        n_in = inputs.get_shape()[-1]
        kernel = tf_shim.Variable(tf_shim.contrib.layers.xavier_initializer()([n_in, units]), name="kernel")
        bias = tf_shim.Variable(np.zeros(units, np.float32), name="bias")
        out = T(lambda a, k, b: a @ k + b, [inputs, kernel, bias])
        return activation(out) if activation is not None else out

    def conv1d(inputs, filters, kernel_size, activation=None, use_bias=True, **_):
        """layers.conv1d, stride 1, 'valid': kernel [kernel_size, in, filters], then bias [filters]; with kernel_size 1
        every position is inputs[t] kernel[0] + bias"""
        assert kernel_size == 1 and use_bias
        n_in = inputs.get_shape()[-1]
        kernel = tf_shim.Variable(tf_shim.contrib.layers.xavier_initializer()([1, n_in, filters]), name="kernel")
        bias = tf_shim.Variable(np.zeros(filters, np.float32), name="bias")
        out = T(lambda a, k, b: a @ k[0] + b, [inputs, kernel, bias])
        return activation(out) if activation is not None else out

    def dropout(inputs, rate=0.5, noise_shape=None, seed=None, training=False, name=None):
        """layers.dropout -> nn.dropout(x, keep_prob = 1 - rate) while training: div(x, keep_prob) * binary; a
        keep_prob of 1 returns x (no draw).  The {0, 1} mask is drawn through the session (inject / draw_log)."""
        keep = 1.0 - float(rate)

        def f(a, tr):
            if not bool(tr) or keep == 1.0:
                return a
            m = tf_shim._RUN["session"].draw("dropout", tuple(a.shape), keep_prob=keep)
            return (a / keep) * tf_shim._to_torch(m).to(a.dtype)
        return T(f, [inputs, training])

    def tile(x, multiples, name=None):
        return T(lambda a, *ms: a.repeat(*[int(m) for m in ms]), [x] + _dims(multiples))

    def reshape(x, shape, name=None):
        return T(lambda a, *ss: a.reshape(*[int(s) for s in ss]), [x] + _dims(shape))

    def where(cond, x, y, name=None):
        return T(lambda c, a, b: torch.where(c, a, b), [cond, x, y])

    def split(value, num_or_size_splits, axis=0, name=None):
        """array_ops.split with an int: that many equal pieces; a size that does not divide raises"""
        if not isinstance(num_or_size_splits, int):
            return tf_shim._sasrec_split(value, num_or_size_splits, axis)
        n = num_or_size_splits
        size = value.get_shape()[axis]
        if size % n:
            raise ValueError("Dimension size must be evenly divisible by %d but is %d" % (n, size))

        def piece(i):
            return T(lambda a: a.narrow(axis, i * (a.shape[axis] // n), a.shape[axis] // n), [value])
        return [piece(i) for i in range(n)]

    if not hasattr(tf_shim, "_sasrec_split"):
        tf_shim._sasrec_split = tf_shim.split

    class LinearOperatorLowerTriangular:
        """linalg.LinearOperatorLowerTriangular(tril).to_dense(): the lower triangle of `tril`, the rest zero"""

        def __init__(self, tril, **_):
            self.tril = tril

        def to_dense(self):
            return T(lambda a: torch.tril(a), [self.tril])

    tf_shim.get_collection, tf_shim.get_variable, tf_shim.add_n = get_collection, get_variable, add_n
    tf_shim.nn.moments = moments
    tf_shim.layers = types.SimpleNamespace(dense=dense, conv1d=conv1d, dropout=dropout)
    tf_shim.sign = lambda x, name=None: T(torch.sign, [x])
    tf_shim.abs = lambda x, name=None: T(torch.abs, [x])
    tf_shim.ones = lambda shape, dtype=None, **_: T(
        lambda: torch.ones(*[int(s) for s in shape], dtype=tf_shim.float_dtype()), [])
    tf_shim.ones_like = lambda x, name=None, **_: T(torch.ones_like, [x])
    tf_shim.equal = lambda a, b, name=None: T(lambda x, y: x == y, [a, b])
    tf_shim.not_equal = lambda a, b, name=None: T(lambda x, y: x != y, [a, b])
    tf_shim.to_float = lambda x, name=None: T(lambda a: a.to(tf_shim.float_dtype()), [x])
    tf_shim.range = lambda n, name=None: T(lambda k: torch.arange(int(k)), [n])
    tf_shim.convert_to_tensor = lambda x, **_: x if isinstance(x, T) else tf_shim._Const(x)
    tf_shim.tile, tf_shim.reshape, tf_shim.where, tf_shim.split = tile, reshape, where, split
    tf_shim.linalg = types.SimpleNamespace(LinearOperatorLowerTriangular=LinearOperatorLowerTriangular)
    return check_sasrec_ops()


def check_sasrec_ops():
    """every attached op on a small hand-computed value"""
    import torch
    tf = tf_shim
    run = lambda t: tf._evaluate([t], {})[0]
    tf.set_float("float64")
    tf.reset_default_graph()
    tf._GRAPH.collections = {}
    x = tf.constant(np.asarray([[1.0, -2.0, 3.0], [0.0, 0.0, 0.0]]))
    mean, var = tf.nn.moments(x, [-1], keep_dims=True)
    assert run(mean).tolist() == [[2.0 / 3.0], [0.0]]
    assert abs(float(run(var)[0, 0]) - (((1 - 2 / 3) ** 2 + (-2 - 2 / 3) ** 2 + (3 - 2 / 3) ** 2) / 3)) < 1e-15
    assert run(tf.sign(tf.abs(tf.reduce_sum(x, axis=-1)))).tolist() == [1.0, 0.0]
    assert run(tf.tile(tf.expand_dims(tf.constant(np.asarray([1.0, 2.0])), 0), [2, 1])).tolist() == [[1.0, 2.0]] * 2
    assert run(tf.tile(tf.constant(np.asarray([[1.0, 2.0]])), [tf.shape(x)[0], 2])).tolist() == [[1.0, 2.0, 1.0, 2.0]] * 2
    assert run(tf.ones_like(x)).tolist() == [[1.0] * 3] * 2 and run(tf.ones([2])).tolist() == [1.0, 1.0]
    pad = tf.ones_like(x) * (-2 ** 32 + 1)
    assert run(tf.where(tf.equal(x, 0), pad, x)).tolist() == [[1.0, -2.0, 3.0], [-4294967295.0] * 3]
    assert run(tf.to_float(tf.not_equal(tf.constant(np.asarray([3, 5, 3])), 3))).tolist() == [0.0, 1.0, 0.0]
    assert run(tf.range(tf.shape(x)[1])).tolist() == [0, 1, 2]
    assert run(tf.reshape(x, [tf.shape(x)[0] * 3])).tolist() == [1.0, -2.0, 3.0, 0.0, 0.0, 0.0]
    sq = tf.constant(np.asarray([[1.0, 2.0], [3.0, 4.0]]))
    assert run(tf.linalg.LinearOperatorLowerTriangular(sq).to_dense()).tolist() == [[1.0, 0.0], [3.0, 4.0]]
    sm = run(tf.nn.softmax(tf.constant(np.asarray([[0.0, np.log(3.0)]]))))
    assert np.abs(sm.numpy() - [[0.25, 0.75]]).max() < 1e-15
    flag = tf.convert_to_tensor(tf.placeholder(tf.bool, name="flag"))
    assert isinstance(flag, tf.Tensor)
    y3 = tf.constant(np.arange(12.0).reshape(1, 2, 6))
    a, b = tf.split(y3, 2, axis=2)
    assert run(tf.concat([a, b], axis=0)).tolist() == [[[0.0, 1.0, 2.0], [6.0, 7.0, 8.0]],
                                                       [[3.0, 4.0, 5.0], [9.0, 10.0, 11.0]]]
    try:
        tf.split(y3, 4, axis=2)
        raise AssertionError("split 6 into 4")
    except ValueError:
        pass
    assert y3.get_shape().as_list() == [1, 2, 6] and list(y3.get_shape()[-1:]) == [6]
    # dense / conv1d: kernel then bias, x k + b
    n0 = len(tf._GRAPH.variables)
    d = tf.layers.dense(x, 2, activation=None)
    c = tf.layers.conv1d(inputs=tf.expand_dims(x, 0), filters=2, kernel_size=1, activation=tf.nn.relu, use_bias=True)
    kd, bd, kc, bc = tf._GRAPH.variables[n0:]
    assert tuple(kd.value.shape) == (3, 2) and tuple(bd.value.shape) == (2,) and tuple(kc.value.shape) == (1, 3, 2)
    kd.load(np.asarray([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]))
    bd.load(np.asarray([0.5, -0.5]))
    kc.load(np.asarray([[[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]]))
    bc.load(np.asarray([0.5, -0.5]))
    assert run(d).tolist() == [[4.5, 0.5], [0.5, -0.5]]
    assert run(c).tolist() == [[[4.5, 0.5], [0.5, 0.0]]]
    # dropout: x / keep * mask while training, x otherwise; a rate of 0 draws nothing
    sess = tf.Session(seed=0)
    tr = tf.placeholder(tf.bool, name="training_flag")
    dr = tf.layers.dropout(x, rate=0.5, training=tf.convert_to_tensor(tr))
    sess.inject([np.asarray([[1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])])
    assert sess.run(dr, feed_dict={tr: True}).tolist() == [[2.0, 0.0, 6.0], [0.0, 0.0, 0.0]]
    assert sess.run(dr, feed_dict={tr: False}).tolist() == run(x).tolist() and len(sess.draw_log) == 1
    assert sess.run(tf.layers.dropout(x, rate=0, training=tf.convert_to_tensor(tr)), feed_dict={tr: True}).tolist() == \
        run(x).tolist() and len(sess.draw_log) == 1
    # get_variable + the regulariser collection; add_n of nothing raises
    tf._GRAPH.collections = {}
    v = tf.get_variable("v", dtype=tf.float32, shape=[2, 2], regularizer=tf.contrib.layers.l2_regularizer(0.5))
    v.load(np.asarray([[1.0, 2.0], [3.0, 4.0]]))
    pens = tf.get_collection(tf.GraphKeys.REGULARIZATION_LOSSES)
    assert len(pens) == 1 and float(run(tf.add_n(pens))) == 0.5 * 30.0 / 2
    tf._GRAPH.collections = {}
    tf.get_variable("w", dtype=tf.float32, shape=[2, 2], regularizer=tf.contrib.layers.l2_regularizer(0.0))
    assert tf.get_collection(tf.GraphKeys.REGULARIZATION_LOSSES) == []
    try:
        tf.add_n([])
        raise AssertionError("add_n([])")
    except ValueError:
        pass
    with tf.variable_scope("scope", reuse=None):
        pass
    tf._GRAPH.collections = {}
    tf.reset_default_graph()
    return True


def build(dataset, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    tf_shim._GRAPH.collections = {}
    mod = load_sasrec()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "SASRec"
    conf.update(hyper)
    sess = G.RecordingSession(seed=0)
    model = mod.SASRec(sess, dataset, conf)
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess


def _hyper(case, batch, rate=None):
    d, h, nb, L, l2, r = P.CASES[case]
    return dict(lr=P.LR, l2_emb=l2, hidden_units=d, dropout_rate=r if rate is None else rate, max_len=L, num_blocks=nb,
                num_heads=h, batch_size=batch, epochs=1, topk=20)


def _load(variables, names, init):
    assert len(variables) == len(names), (len(variables), len(names))
    for var, n in zip(variables, names):
        t = init[n]
        var.load(t.reshape(var.value.shape))              # conv1d kernels are [1, d, d]


def _tabs(variables, names, init):
    return [v.numpy().reshape(init[n].shape) for v, n in zip(variables, names)]


def make_feeds(model, I, L, steps, B, seed):
    """3 batches of B rows out of get_train_data(): every kind of row in each — truncated, exactly full, short,
    all-padded (a one-item user)"""
    np.random.seed(seed)
    seq, pos, neg = (np.asarray(a, np.int32) for a in model.get_train_data())
    n_real = (seq != I).sum(1)
    kinds = {"empty": np.flatnonzero(n_real == 0), "one": np.flatnonzero(n_real == 1),
             "short": np.flatnonzero((n_real > 1) & (n_real < L)), "full": np.flatnonzero(n_real == L)}
    lens = np.asarray([len(model.user_pos_train[u]) for u in model.user_pos_train])
    kinds["truncated"] = np.flatnonzero(lens - 1 > L)
    kinds["exact"] = np.flatnonzero(lens - 1 == L)
    for k, v in kinds.items():
        assert len(v), "no %s row at max_len %d" % (k, L)
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        rows = [int(rs.choice(v)) for v in kinds.values()]
        rest = np.setdiff1d(np.arange(len(seq)), rows)
        rows += rs.choice(rest, B - len(rows), replace=False).tolist()
        rows = np.asarray(rows)[rs.permutation(B)]
        out.append((seq[rows], pos[rows], neg[rows]))
    return out


def run_case(ds, case, init, feeds, with_predict=None):
    d, h, nb, L, l2, rate = P.CASES[case]
    names = P.table_names(nb)
    out = {}
    masks = None
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, _hyper(case, B_STEP), width)
        variables = list(tf_shim._GRAPH.variables)
        _load(variables, names, init)
        tabs, losses, logs = [], [], []
        for k, (seq, pos, neg) in enumerate(feeds):
            feed = {model.item_seq_ph: seq, model.item_pos_ph: pos, model.item_neg_ph: neg, model.is_training: True}
            if masks is not None:
                sess.inject([m for m in masks[k]])       # the f64 twin takes the f32 run's masks
            n0 = len(sess.draw_log)
            _, loss = sess.run([model.train_opt, model.loss], feed_dict=feed)
            logs.append([a for _, a in sess.draw_log[n0:]])
            losses.append(float(loss))
            tabs.append(_tabs(variables, names, init))
        if masks is None:
            masks = logs
        assert all(len(m) == (P.n_sites(nb) if rate else 0) for m in logs)
        out[tag] = (tabs, losses)
        if with_predict is not None:
            users, cand = with_predict
            out[tag + "_predict"] = _np(model.predict(list(users), None), width)
            out[tag + "_predict_cand"] = _np(model.predict(list(users), [list(c) for c in cand]), width)
            bat = model_pad(model, users)
            emb = sess.run(model.seq, feed_dict={model.item_seq_ph: bat, model.is_training: False})
            out[tag + "_user_emb"] = _np(emb[:, -1, :], width)
    out["masks"] = masks
    return out


def model_pad(model, users):
    from oracle import ref_models                       # noqa: F401  (the tool module is the reference's)
    rows = [model.user_pos_train[u] for u in users]
    out = np.full((len(rows), model.max_len), model.items_num, np.int32)
    for r, s in enumerate(rows):
        cut = s[-model.max_len:]
        out[r, model.max_len - len(cut):] = cut
    return out


def pack_tables(case, names, tabs_by_tag, init):
    out = {}
    for j, name in enumerate(names):
        i64 = init[name].astype(np.float64)
        if name == "item_emb":
            moved = np.zeros(len(i64), bool)
            for tabs in tabs_by_tag.values():
                for t in tabs:
                    moved |= (t[j].astype(np.float64) != i64).any(axis=1)
            rows = np.flatnonzero(moved).astype(np.int32)
            out["%s_rows_item_emb" % case] = rows
        else:
            rows = slice(None)
        for tag, width in WIDTHS:
            delta = np.stack([t[j].astype(np.float64)[rows] - i64[rows] for t in tabs_by_tag[tag]])
            back = i64[rows][None] + delta.astype(np.float32).astype(np.float64)
            want = np.stack([t[j][rows] for t in tabs_by_tag[tag]]).astype(np.float64)
            assert np.abs(back - want).max(initial=0) <= 2.0 ** -24 * np.abs(delta).max(initial=0)
            out["%s_%s_%s" % (case, tag, name)] = delta.astype(np.float32)
    return out


def run_epoch(ds, init):
    case = "first"
    d, h, nb, L, l2, _ = P.CASES[case]
    names = P.table_names(nb)
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, _hyper(case, B_EPOCH, rate=0.0), width)
        variables = list(tf_shim._GRAPH.variables)
        _load(variables, names, init)
        np.random.seed(EPOCH_SEED)
        sess.feed_log = []
        model.train_model()
        feeds = [f for f in sess.feed_log if "item_pos" in f]
        sess.feed_log = None
        out[tag] = dict(feeds=feeds, tabs=[_tabs(variables, names, init)])
    a, b = out["f32"]["feeds"], out["f64"]["feeds"]
    assert len(a) == len(b) and all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in ("item_seq", "item_neg"))
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    G.attach_ops()
    attach_sasrec_ops()
    R = toy_matrix(isolated=False)
    U, I = R.shape
    seqs = time_orders(R)
    ds = TimedDataset(R, seqs)
    ptr = np.zeros(U + 1, np.int64)
    for u, s in seqs.items():
        ptr[u + 1] = len(s)
    ptr = np.cumsum(ptr)
    out = dict(indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32), shape=np.asarray(R.shape, np.int64),
               seq_ptr=ptr, seq=np.asarray([i for u in sorted(seqs) for i in seqs[u]], np.int32),
               lr=np.float64(P.LR), cases=np.asarray(sorted(P.CASES)), batch_step=np.int64(B_STEP),
               batch_epoch=np.int64(B_EPOCH))
    lens = np.diff(ptr)
    order = np.argsort(-lens, kind="stable")
    present = [u for u in order if lens[u] > 0]
    predict_users = np.asarray([present[0], present[1], present[len(present) // 2], present[-1], present[3]], np.int32)
    cand = np.asarray([[3, 0, I - 1], [7, 7, 1], [0, 1, 2], [I - 1, I - 2, 5], [9, 8, 0]], np.int32)
    out.update(predict_users=predict_users, predict_cand=cand)
    gaps = {}
    for k, case in enumerate(sorted(P.CASES)):
        d, h, nb, L, l2, rate = P.CASES[case]
        names = P.table_names(nb)
        init = P.init_tables(I, d, L, nb, seed=900 + k)
        model, _ = build(ds, _hyper(case, B_STEP), "float64")
        feeds = make_feeds(model, I, L, STEPS, B_STEP, FEED_SEED + k)
        last = case == P.PREDICT_CASE
        res = run_case(ds, case, init, feeds, (predict_users, cand) if last else None)
        for n in names:
            out["%s_init_%s" % (case, n)] = init[n]
        for j, nm in enumerate(("seq", "pos", "neg")):
            out["%s_%s" % (case, nm)] = np.stack([f[j] for f in feeds]).astype(np.int32)
        if rate:
            for s in range(P.n_sites(nb)):
                out["%s_mask%d" % (case, s)] = np.stack([m[s] for m in res["masks"]]).astype(np.uint8)
        for tag, _ in WIDTHS:
            out["%s_loss_%s" % (case, tag)] = np.asarray(res[tag][1], np.float64)
        out.update(pack_tables(case, names, {tag: res[tag][0] for tag, _ in WIDTHS}, init))
        if last:
            for tag, _ in WIDTHS:
                out["user_emb_" + tag] = res[tag + "_user_emb"]
                out["predict_" + tag] = res[tag + "_predict"]
                out["predict_cand_" + tag] = res[tag + "_predict_cand"]
        gaps[case] = max(np.abs(out["%s_f32_%s" % (case, t)].astype(np.float64) - out["%s_f64_%s" % (case, t)]).max()
                         for t in names)
    # one whole epoch of train_model()
    d, h, nb, L, l2, _ = P.CASES["first"]
    names = P.table_names(nb)
    init = P.init_tables(I, d, L, nb, seed=990)
    ep = run_epoch(ds, init)
    feeds = ep["f64"]["feeds"]
    S = len(feeds)
    eseq, epos, eneg = (np.full((S, B_EPOCH, L), I, np.int32) for _ in range(3))
    rows = np.zeros(S, np.int32)
    for s, f in enumerate(feeds):
        n = len(f["item_seq"])
        rows[s] = n
        eseq[s, :n], epos[s, :n], eneg[s, :n] = f["item_seq"], f["item_pos"], f["item_neg"]
    for n in names:
        out["epoch_init_%s" % n] = init[n]
    out.update(epoch_seq=eseq, epoch_pos=epos, epoch_neg=eneg, epoch_rows=rows, epoch_seed=np.int64(EPOCH_SEED))
    out.update(pack_tables("epoch", names, {tag: ep[tag]["tabs"] for tag, _ in WIDTHS}, init))
    gaps["epoch"] = max(np.abs(out["epoch_f32_%s" % t].astype(np.float64) - out["epoch_f64_%s" % t]).max()
                        for t in names)
    path = os.path.join(HERE, "tfgraph_sasrec.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); %d epoch steps; fp32 vs fp64 table gaps %s; predict gap %.3g" % (
        path, os.path.getsize(path), S, {k: "%.3g" % v for k, v in gaps.items()},
        np.abs(out["predict_f32"] - out["predict_f64"]).max()))


if __name__ == "__main__":
    main()
