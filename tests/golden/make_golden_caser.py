"""Golden Caser trace produced by the REFERENCE's own Caser class (model/sequential_recommender/Caser.py).

The class is loaded whole and unchanged with oracle/ref_models._load_file and runs under oracle/tf_shim.py, as
make_golden_sasrec.py loads its class.  Ops of Caser.py the shim lacks are attached from here (attach_caser_ops, on top
of make_golden_sasrec.attach_sasrec_ops) by their published definitions [EXT: tensorflow r1.12], each checked on a small
hand-computed value before use — the even split of reduce_max's gradient between tied positions among them.

Stand-ins for the surroundings, as in the other makers: `util.DataIterator`, `pad_sequences` and
`csr_to_user_dict_bytime` are the reference's own files; `batch_randint_choice` (Cython over glibc rand() in the
reference) is caser_restatement's numpy-stream sampler.

The cases hold no pad target: a gather of row I from a table of I rows raises under the shim as it does under TF on a
CPU.  The recorded epoch runs every user of the toy data, some with fewer than seq_T items, so it is run with the
gather of TF on a GPU [EXT: tf.gather, "On GPU, if an out of bound index is found, a 0 is stored in the corresponding
output value"], attached for that run only (gpu_gather).

    python tests/golden/make_golden_caser.py              # needs the reference tree

Writes tests/golden/tfgraph_caser.npz:
  indptr / indices / shape     the train pattern: toy_matrix(isolated=False) (157 x 131)
  seq_ptr / seq                every user's items by time: a seeded permutation of the row (make_golden_fpmc)
  <case>_init_seed             the initial variables of the case are caser_restatement.init_tables(157, 131, ..., seed)
                               (numpy's legacy RandomState: the same values on every machine)
  <case>_users / _seq / _pos / _neg   [steps, B], [steps, B, L], [steps, B, T], [steps, B, N] the feeds
  <case>_mask                  [steps, B, F] uint8: the dropout mask of every step, from the session's draw_log (rate > 0)
  <case>_loss_{f32,f64}        [steps] the loss fetched with each step (before its update)
  <case>_f64_<var>             [steps, ...]: the variable after each step of the float64 run MINUS its initial value,
                               stored as float32: the differences are ~1e-3 and lose at most 2^-24 of that, four orders
                               below the tolerance that reads them
  <case>_gap_<var>             [steps]: max |float32 run - float64 run| of the variable after each step, the reference's
                               own distance between the widths
  epoch_*                      one train_model() epoch of the case `first` at batch_size 16, rate 0, with a recording
                               session: epoch_users / _seq / _pos / _neg [S, 16, .] (the last batch filled up, epoch_rows
                               [S] its true size), epoch_seed, the end tables under the case name `epoch`
  predict_users, predict_{f32,f64}, predict_cand, predict_cand_{f32,f64}
                               predict() after the last step of the case `second`, full and candidate mode
"""
import builtins
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
import make_golden_sasrec as S                # noqa: E402
import caser_restatement as P                 # noqa: E402

B_STEP, B_EPOCH, STEPS = 20, 16, 3
EPOCH_SEED = 5244
FEED_SEED = 5245


def load_caser():
    """the reference module model/sequential_recommender/Caser.py, executed under the shim"""
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
        mod = rm._load_file("model.sequential_recommender.Caser",
                            os.path.join(rm.REF, "model", "sequential_recommender", "Caser.py"))
        sys.modules.pop("model.sequential_recommender.Caser", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


# ------------------------------------------------------------------ the ops Caser.py needs beyond the shim's and SASRec's
def _activation(a):
    """keras.activations.get: None, a callable, or a name"""
    if a is None or callable(a):
        return a
    return {"relu": tf_shim.nn.relu}[a]


def attach_caser_ops():
    import torch
    T = tf_shim.Tensor
    S.attach_sasrec_ops()
    glorot = tf_shim.contrib.layers.xavier_initializer

    class Conv2D:
        """layers.Conv2D(filters, kernel_size): strides 1, 'valid', channels last.  The variables are made at the first
        call: kernel [height, width, in, filters] (glorot uniform), then bias [filters] (zeros).
        out[b, p, q, c] = bias[c] + sum_{t, s, i} in[b, p + t, q + s, i] kernel[t, s, i, c], then the activation"""

        def __init__(self, filters, kernel_size, activation=None, **_):
            self.filters, self.size, self.act, self.vars = int(filters), [int(k) for k in kernel_size], \
                _activation(activation), None

        def __call__(self, inputs):
            if self.vars is None:
                n_in = inputs.get_shape()[-1]
                self.vars = (tf_shim.Variable(glorot()(self.size + [n_in, self.filters]), name="kernel"),
                             tf_shim.Variable(np.zeros(self.filters, np.float32), name="bias"))

            def f(a, k, b):
                out = torch.nn.functional.conv2d(a.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1))
                return out.permute(0, 2, 3, 1) + b
            out = T(f, [inputs, self.vars[0], self.vars[1]])
            return self.act(out) if self.act is not None else out

    class Dense:
        """layers.Dense(units): at the first call kernel [in, units] (glorot uniform), then bias [units] (zeros);
        activation(inputs kernel + bias)"""

        def __init__(self, units, activation=None, **_):
            self.units, self.act, self.vars = int(units), _activation(activation), None

        def __call__(self, inputs):
            if self.vars is None:
                n_in = inputs.get_shape()[-1]
                self.vars = (tf_shim.Variable(glorot()([n_in, self.units]), name="kernel"),
                             tf_shim.Variable(np.zeros(self.units, np.float32), name="bias"))
            out = T(lambda a, k, b: a @ k + b, [inputs, self.vars[0], self.vars[1]])
            return self.act(out) if self.act is not None else out

    class Dropout:
        """layers.Dropout(rate): layers.dropout at the call"""

        def __init__(self, rate=0.5, **_):
            self.rate = rate

        def __call__(self, inputs, training=False):
            return tf_shim.layers.dropout(inputs, rate=self.rate, training=training)

    def reduce_max(x, axis=None, keepdims=False, name=None, **_):
        """math_ops.reduce_max; its gradient (_MinOrMaxGrad) is split EVENLY between the positions that equal the
        maximum — torch.amax's rule too"""
        return T(lambda a: torch.amax(a, dim=int(axis), keepdim=bool(keepdims)), [x])

    tf_shim.layers.Conv2D, tf_shim.layers.Dense, tf_shim.layers.Dropout = Conv2D, Dense, Dropout
    tf_shim.reduce_max = reduce_max
    int_split = tf_shim.split

    def split(value, num_or_size_splits, axis=0, name=None):
        """array_ops.split with a list of sizes: consecutive pieces of those sizes along `axis` (make_golden_sasrec's
        handles a count; the shim's own list form reads the module's `range`, which attach_sasrec_ops replaces)"""
        if isinstance(num_or_size_splits, int):
            return int_split(value, num_or_size_splits, axis)
        sizes = [int(s) for s in num_or_size_splits]
        offs = [sum(sizes[:k]) for k in builtins.range(len(sizes))]
        return [T(lambda a, lo=lo, n=n: a.narrow(axis, lo, n), [value]) for lo, n in zip(offs, sizes)]
    tf_shim.split = split

    def matmul(a, b, transpose_a=False, transpose_b=False, name=None):
        """math_ops.matmul on batches of matrices: the transposes swap the LAST two dimensions (the shim's own is
        written for two-dimensional inputs)"""
        def f(x, y):
            x = x.transpose(-1, -2) if transpose_a else x
            y = y.transpose(-1, -2) if transpose_b else y
            return x @ y
        return T(f, [a, b])
    tf_shim.matmul = matmul
    # init_ops.Zeros: initializer(shape) -> zeros
    tf_shim.initializers = types.SimpleNamespace(zeros=lambda dtype=None: (lambda shape, dtype=None, partition_info=None:
                                                                         np.zeros([int(s) for s in shape], np.float32)))
    return check_caser_ops()


def gpu_gather(on):
    """tf.gather / embedding_lookup as TF on a GPU run them: an index outside the table reads zeros.  on=False puts the
    shim's own (which raise, as TF on a CPU does) back"""
    import torch
    if not hasattr(tf_shim, "_caser_lookup"):
        tf_shim._caser_lookup = (tf_shim.nn.embedding_lookup, tf_shim.gather)
    if not on:
        tf_shim.nn.embedding_lookup, tf_shim.gather = tf_shim._caser_lookup
        return

    def lookup(params, ids, name=None, **_):
        def f(p, i):
            padded = torch.cat([p, torch.zeros((1,) + tuple(p.shape[1:]), dtype=p.dtype)], dim=0)
            flat = i.reshape(-1)
            flat = torch.where((flat < 0) | (flat >= p.shape[0]), torch.full_like(flat, p.shape[0]), flat)
            return padded.index_select(0, flat).reshape(tuple(i.shape) + tuple(p.shape[1:]))
        return tf_shim.Tensor(f, [params, ids], kind="gather")
    tf_shim.nn.embedding_lookup = tf_shim.gather = lookup


def check_caser_ops():
    """every attached op on a small hand-computed value"""
    import torch
    tf = tf_shim
    run = lambda t: tf._evaluate([t], {})[0]
    tf.set_float("float64")
    tf.reset_default_graph()
    tf._GRAPH.collections = {}
    # Conv2D: a vertical kernel [2, 1, 1, 2] over a 2 x 3 image, then a horizontal one [1, 3, 1, 1] with relu
    img = tf.constant(np.asarray([[1.0, 2.0, 3.0], [4.0, 5.0, -20.0]]).reshape(1, 2, 3, 1))
    n0 = len(tf._GRAPH.variables)
    cv, ch = tf.layers.Conv2D(2, [2, 1]), tf.layers.Conv2D(1, [1, 3], activation="relu")
    assert len(tf._GRAPH.variables) == n0                      # nothing is made before the first call
    ov, oh = cv(img), ch(img)
    kv, bv, kh, bh = tf._GRAPH.variables[n0:]
    assert tuple(kv.value.shape) == (2, 1, 1, 2) and tuple(bv.value.shape) == (2,) and tuple(kh.value.shape) == (1, 3, 1, 1)
    kv.load(np.asarray([[1.0, 10.0], [2.0, -1.0]]).reshape(2, 1, 1, 2))
    bv.load(np.asarray([0.5, 0.0]))
    kh.load(np.asarray([1.0, 1.0, 1.0]).reshape(1, 3, 1, 1))
    bh.load(np.asarray([1.0]))
    # out_v[0, 0, j, c] = b[c] + x[0][j] K[0][c] + x[1][j] K[1][c]
    assert run(ov).tolist() == [[[[9.5, 6.0], [12.5, 15.0], [-36.5, 50.0]]]]
    assert run(tf.reshape(ov, [1, 6])).tolist() == [[9.5, 6.0, 12.5, 15.0, -36.5, 50.0]]      # feature j nv + c
    assert run(oh).tolist() == [[[[7.0]], [[0.0]]]]                                          # relu(1 - 11) = 0
    assert run(tf.reduce_max(tf.squeeze(oh, axis=2), axis=1)).tolist() == [[7.0]]
    # reduce_max's gradient: an even split between ties
    leaf = torch.tensor([[1.0, 3.0, 3.0], [2.0, 0.0, 1.0]], dtype=torch.float64, requires_grad=True)
    v = tf.Variable(leaf.detach().numpy())
    out = tf._evaluate([tf.reduce_max(v, axis=1)], {}, {id(v): leaf})[0]
    out.sum().backward()
    assert out.tolist() == [3.0, 2.0] and leaf.grad.tolist() == [[0.0, 0.5, 0.5], [1.0, 0.0, 0.0]]
    # Dense with relu; Dropout through the session
    x = tf.constant(np.asarray([[1.0, -2.0, 3.0]]))
    n0 = len(tf._GRAPH.variables)
    dl = tf.layers.Dense(2, activation="relu")
    od = dl(x)
    kd, bd = tf._GRAPH.variables[n0:]
    kd.load(np.asarray([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]))
    bd.load(np.asarray([0.5, -1.5]))
    assert run(od).tolist() == [[4.5, 0.0]]
    sess = tf.Session(seed=0)
    tr = tf.placeholder(tf.bool, name="training_flag")
    dr = tf.layers.Dropout(0.5)(x, training=tr)
    sess.inject([np.asarray([[1.0, 0.0, 1.0]])])
    assert sess.run(dr, feed_dict={tr: True}).tolist() == [[2.0, 0.0, 6.0]]
    assert sess.run(dr, feed_dict={tr: False}).tolist() == [[1.0, -2.0, 3.0]] and len(sess.draw_log) == 1
    a, b = tf.split(tf.constant(np.asarray([[1.0, 2.0, 3.0, 4.0, 5.0]])), [2, 3], axis=1)
    assert run(a).tolist() == [[1.0, 2.0]] and run(b).tolist() == [[3.0, 4.0, 5.0]]
    m3 = tf.matmul(tf.constant(np.asarray([[[1.0, 2.0]]])), tf.constant(np.asarray([[[3.0, 4.0], [5.0, 6.0]]])),
                   transpose_b=True)
    assert run(m3).tolist() == [[[11.0, 17.0]]]
    zv = tf.get_variable("z",dtype=tf.float32, shape=[3], initializer=tf.initializers.zeros())
    assert zv.numpy().tolist() == [0.0, 0.0, 0.0]
    # gather: the shim's raises outside the table; the GPU reading gives zeros
    tab = tf.Variable(np.asarray([[1.0, 2.0], [3.0, 4.0]]))
    ids = tf.constant(np.asarray([1, 2]))
    try:
        run(tf.nn.embedding_lookup(tab, ids))
        raise AssertionError("a gather outside the table")
    except (IndexError, RuntimeError):
        pass
    gpu_gather(True)
    try:
        got = tf.gather(tab, ids)
        assert got.kind == "gather" and run(got).tolist() == [[3.0, 4.0], [0.0, 0.0]]
    finally:
        gpu_gather(False)
    tf._GRAPH.collections = {}
    tf.reset_default_graph()
    return True


def build(dataset, hyper, width, on_gpu=False):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    tf_shim._GRAPH.collections = {}
    mod = load_caser()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "Caser"
    conf.update(hyper)
    sess = G.RecordingSession(seed=0)
    model = mod.Caser(sess, dataset, conf)
    gpu_gather(on_gpu)
    try:
        model.build_graph()
    finally:
        gpu_gather(False)
    sess.run(tf_shim.global_variables_initializer())
    model.user_pos_train = mod.csr_to_user_dict_bytime(dataset.time_matrix, dataset.train_matrix)
    return model, sess


def _hyper(case, batch, rate=None):
    d, L, T, N, nv, nh, l2, r = P.CASES[case]
    return dict(lr=P.LR, l2_reg=l2, factors_num=d, seq_L=L, seq_T=T, nv=nv, nh=nh, dropout=r if rate is None else rate,
                neg_samples=N, batch_size=batch, epochs=1, topk=20)


def _load(variables, names, init):
    assert len(variables) == len(names), (len(variables), len(names))
    for var, n in zip(variables, names):
        var.load(init[n].reshape(var.value.shape))        # the conv kernels are [h, w, 1, filters]


def _tabs(variables, names, init):
    return [v.numpy().reshape(init[n].shape) for v, n in zip(variables, names)]


def make_feeds(model, I, L, N, steps, B, seed, padded_share):
    """`steps` batches of B rows out of _generate_sequences(): in each a full window, a one-pad row, a mostly-pad row
    and a user twice; no pad target.  The long users' many windows would crowd the short users' single rows out:
    `padded_share` of a batch is drawn from the front-padded rows first"""
    users, seq, pos = (np.asarray(a, np.int32) for a in model._generate_sequences())
    ok = (pos != I).all(axis=1)
    n_pad = (seq != I).sum(1)
    n_pad = L - n_pad
    kinds = {"full": np.flatnonzero(ok & (n_pad == 0)), "one": np.flatnonzero(ok & (n_pad == 1)),
             "mostly": np.flatnonzero(ok & (n_pad >= max(1, (L + 1) // 2)))}
    for k, v in kinds.items():
        assert len(v), "no %s row at seq_L %d" % (k, L)
    counts = np.bincount(users[ok])
    twice = np.flatnonzero(counts >= 2)
    assert len(twice)
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        u2 = int(rs.choice(twice))
        rows = rs.choice(np.flatnonzero(ok & (users == u2)), 2, replace=False).tolist()
        rows += [int(rs.choice(v)) for v in kinds.values()]
        padded = np.setdiff1d(np.flatnonzero(ok & (n_pad > 0)), rows)         # one row per short user
        n_padded = min(len(padded), int(round(padded_share * B)))
        rows += rs.choice(padded, n_padded, replace=False).tolist()
        rest = np.setdiff1d(np.flatnonzero(ok), rows)
        rows += rs.choice(rest, B - len(rows), replace=False).tolist()
        rows = np.asarray(rows)[rs.permutation(B)]
        neg = np.zeros((B, N), np.int32)
        for r, row in enumerate(rows):
            neg[r] = P.numpy_batch_randint_choice(I, [N], exclusion=[model.user_pos_train[int(users[row])]])[0]
        out.append((users[rows], seq[rows], pos[rows], neg))
    return out


def run_case(ds, case, init, feeds, with_predict=None):
    d, L, T, N, nv, nh, l2, rate = P.CASES[case]
    names = P.table_names(L)
    out = {}
    masks = None
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, _hyper(case, B_STEP), width)
        variables = list(tf_shim._GRAPH.variables)
        _load(variables, names, init)
        tabs, losses, logs = [], [], []
        for k, (users, seq, pos, neg) in enumerate(feeds):
            feed = {model.user_ph: users, model.item_seq_ph: seq, model.item_pos_ph: pos, model.item_neg_ph: neg,
                    model.is_training: True}
            if masks is not None and rate:
                sess.inject([masks[k]])                  # the f64 twin takes the f32 run's masks
            n0 = len(sess.draw_log)
            _, loss = sess.run([model.train_opt, model.train_opt.loss], feed_dict=feed)
            drawn = [a for _, a in sess.draw_log[n0:]]
            assert len(drawn) == (1 if rate else 0)
            logs.append(drawn[0] if rate else None)
            losses.append(float(loss))
            tabs.append(_tabs(variables, names, init))
        if masks is None:
            masks = logs
        out[tag] = (tabs, losses)
        if with_predict is not None:
            users, cand = with_predict
            model._generate_sequences()                   # user_test_seq
            out[tag + "_predict"] = _np(model.predict(list(users), None), width)
            out[tag + "_predict_cand"] = _np(model.predict(list(users), [list(c) for c in cand]), width)
    out["masks"] = masks
    return out


def pack_tables(case, names, tabs_by_tag, init):
    """the f64 trace as float32 differences from the initial values; of the f32 twin only what the tests read, its
    distance from the f64 trace per step and variable (the whole twin would take the file past the size limit)"""
    out = {}
    for j, name in enumerate(names):
        i64 = init[name].astype(np.float64)
        delta = np.stack([t[j].astype(np.float64) - i64 for t in tabs_by_tag["f64"]])
        back = i64[None] + delta.astype(np.float32).astype(np.float64)
        want = np.stack([t[j] for t in tabs_by_tag["f64"]]).astype(np.float64)
        assert np.abs(back - want).max(initial=0) <= 2.0 ** -24 * np.abs(delta).max(initial=0)
        out["%s_f64_%s" % (case, name)] = delta.astype(np.float32)
        twin = np.stack([t[j] for t in tabs_by_tag["f32"]]).astype(np.float64)
        out["%s_gap_%s" % (case, name)] = np.abs(twin - want).reshape(len(want), -1).max(axis=1)
    return out


def run_epoch(ds, init):
    case = "first"
    L = P.CASES[case][1]
    names = P.table_names(L)
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, _hyper(case, B_EPOCH, rate=0.0), width, on_gpu=True)
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
    attach_caser_ops()
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
        d, L, T, N, nv, nh, l2, rate = P.CASES[case]
        names = P.table_names(L)
        init = P.init_tables(U, I, d, L, nv, nh, seed=700 + k)
        model, _ = build(ds, _hyper(case, B_STEP), "float64")
        np.random.seed(FEED_SEED + k)
        feeds = make_feeds(model, I, L, N, STEPS, B_STEP, FEED_SEED + k, 0.6 if case == "fourth" else 0.25)
        last = case == P.PREDICT_CASE
        res = run_case(ds, case, init, feeds, (predict_users, cand) if last else None)
        out["%s_init_seed" % case] = np.int64(700 + k)
        for j, nm in enumerate(("users", "seq", "pos", "neg")):
            out["%s_%s" % (case, nm)] = np.stack([f[j] for f in feeds]).astype(np.int32)
        if rate:
            out["%s_mask" % case] = np.stack(res["masks"]).astype(np.uint8)
        for tag, _ in WIDTHS:
            out["%s_loss_%s" % (case, tag)] = np.asarray(res[tag][1], np.float64)
        out.update(pack_tables(case, names, {tag: res[tag][0] for tag, _ in WIDTHS}, init))
        if last:
            for tag, _ in WIDTHS:
                out["predict_" + tag] = res[tag + "_predict"]
                out["predict_cand_" + tag] = res[tag + "_predict_cand"]
        gaps[case] = max(out["%s_gap_%s" % (case, t)].max() for t in names)
    # one whole epoch of train_model()
    d, L, T, N, nv, nh, l2, _ = P.CASES["first"]
    names = P.table_names(L)
    init = P.init_tables(U, I, d, L, nv, nh, seed=790)
    ep = run_epoch(ds, init)
    feeds = ep["f64"]["feeds"]
    n_steps = len(feeds)
    eusers = np.zeros((n_steps, B_EPOCH), np.int32)
    eseq, epos = np.full((n_steps, B_EPOCH, L), I, np.int32), np.full((n_steps, B_EPOCH, T), I, np.int32)
    eneg = np.zeros((n_steps, B_EPOCH, N), np.int32)
    rows = np.zeros(n_steps, np.int32)
    for s, f in enumerate(feeds):
        n = len(f["item_seq"])
        rows[s] = n
        eusers[s, :n], eseq[s, :n], epos[s, :n], eneg[s, :n] = f["user"], f["item_seq"], f["item_pos"], f["item_neg"]
    out["epoch_init_seed"] = np.int64(790)
    out.update(epoch_users=eusers, epoch_seq=eseq, epoch_pos=epos, epoch_neg=eneg, epoch_rows=rows,
               epoch_seed=np.int64(EPOCH_SEED))
    out.update(pack_tables("epoch", names, {tag: ep[tag]["tabs"] for tag, _ in WIDTHS}, init))
    gaps["epoch"] = max(out["epoch_gap_%s" % t].max() for t in names)
    path = os.path.join(HERE, "tfgraph_caser.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); %d epoch steps (%d pad targets); fp32 vs fp64 table gaps %s; predict gap %.3g" % (
        path, os.path.getsize(path), n_steps, int((epos == I).sum() - (B_EPOCH - rows[-1]) * T),
        {k: "%.3g" % v for k, v in gaps.items()}, np.abs(out["predict_f32"] - out["predict_f64"]).max()))


if __name__ == "__main__":
    main()
