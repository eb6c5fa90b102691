"""Golden SRGNN trace produced by the REFERENCE's own SRGNN class (model/sequential_recommender/SRGNN.py).

The class is loaded whole and unchanged with oracle/ref_models._load_file and runs under oracle/tf_shim.py, as
make_golden_caser.py loads its class.  Ops of SRGNN.py the shim lacks are attached from here (attach_srgnn_ops, on top of
make_golden_gru4rec.attach_ops — whose GRUCell is the cell — and make_golden_sasrec.attach_sasrec_ops) by their
published definitions [EXT: tensorflow r1.12], each checked on a small hand-computed value before use: gather_nd,
sparse_softmax_cross_entropy_with_logits, to_int32, nn.dynamic_rnn for one time step, train.exponential_decay, an Adam
whose learning rate is a graph node and whose minimize() advances global_step, zeros_initializer and matmul on batches
of matrices.  The shim's integers are int64 throughout; to_int32 truncates and stays int64.

`util.DataIterator` and `pad_sequences` are the reference's own files.

    python tests/golden/make_golden_srgnn.py              # needs the reference tree

Writes tests/golden/tfgraph_srgnn.npz:
  shape, seq_ptr / seq         the toy data (157 x 131): every user's items by time (make_golden_fpmc.time_orders)
  rep_ptr / rep                the hand-made train dict of the case `repeats`
  <case>_init_seed             the initial variables are srgnn_restatement.init_tables(131, d, seed)
  <case>_seq / _target         [steps, B, L] post-padded with I, [steps, B]: the sessions the class was given
  <case>_<s>_adj_in / _adj_out / _alias / _items / _mask    the feed the class itself built for step s
  <case>_lrs                   [steps] the learning rate the optimiser took at each step (float32)
  <case>_loss_{f32,f64}        [steps] the minimize op's .loss fetched with each step (before its update)
  <case>_f64_<var>             the vectors, [steps, ...] float32: the variable after each step of the float64 run MINUS
                               its initial value
  <case>_q_<var>, _scale_<var> the matrices, [steps, ...] int16 and [steps]: the same difference in counts of the step's
                               scale (pack_tables)
  <case>_gap_<var>             [steps]: max |float32 run - float64 run| of the variable after each step
  epoch_*                      one train_model() epoch of `hybrid` at batch_size 16 through a recording session:
                               epoch_order [S, 16] the sample indices in the order the class fed them (checked against
                               the fed targets), epoch_users / epoch_ends the same as (user, end) pairs, epoch_lrs,
                               epoch_seed, the end tables under the case name `epoch`
  predict_users, predict_{f32,f64}, predict_cand, predict_cand_{f32,f64}
                               predict() after the last step of `gated`, full and candidate mode, for 27 users: one full
                               batch of 20 and a padded one
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
import make_golden_sasrec as S                # noqa: E402
import srgnn_restatement as P                 # noqa: E402

B_STEP, B_EPOCH, STEPS = 20, 16, 4
EPOCH_SEED = 6161
FEED_SEED = 6162
N_PREDICT = 27


def load_srgnn():
    """the reference module model/sequential_recommender/SRGNN.py, executed under the shim"""
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
        mod = rm._load_file("model.sequential_recommender.SRGNN",
                            os.path.join(rm.REF, "model", "sequential_recommender", "SRGNN.py"))
        sys.modules.pop("model.sequential_recommender.SRGNN", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


# ------------------------------------------------------------------ the ops SRGNN.py needs beyond the shim's
def exponential_decay_value(learning_rate, global_step, decay_steps, decay_rate, staircase):
    """learning_rate_decay.exponential_decay: global_step and decay_steps cast to the rate's float32; p = global_step /
    decay_steps, floored when staircase; learning_rate * decay_rate ^ p"""
    p = np.float32(int(global_step)) / np.float32(decay_steps)
    if staircase:
        p = np.floor(p)
    return np.float32(np.float32(learning_rate) * np.power(np.float32(decay_rate), p, dtype=np.float32))


def attach_srgnn_ops():
    import torch
    T = tf_shim.Tensor
    G.attach_ops()
    S.attach_sasrec_ops()

    def gather_nd(params, indices, name=None):
        """array_ops.gather_nd: out[k] = params[indices[k][0], indices[k][1], ...]"""
        return T(lambda p, i: p[tuple(i.to(torch.int64).unbind(-1))], [params, indices])

    def sparse_softmax_cross_entropy_with_logits(labels=None, logits=None, name=None):
        """nn_ops: -log_softmax(logits)[labels], the row maximum subtracted first (torch.log_softmax does)"""
        return T(lambda y, z: -torch.log_softmax(z, dim=-1).gather(-1, y.to(torch.int64).unsqueeze(-1)).squeeze(-1),
                 [labels, logits])

    def to_int32(x, name=None):
        """math_ops.to_int32: the cast truncates towards zero"""
        return T(lambda a: torch.trunc(a).to(torch.int64), [x])

    def dynamic_rnn(cell, inputs, initial_state=None, **_):
        """rnn.dynamic_rnn over ONE time step: (outputs [rows, 1, n], final state) = the cell on inputs[:, 0]"""
        shape = inputs.get_shape()
        assert len(shape) == 3 and shape[1] == 1, shape
        h, state = cell(inputs[:, 0, :], initial_state, int(shape[2]))
        return tf_shim.expand_dims(h, 1), state

    def exponential_decay(learning_rate, global_step, decay_steps, decay_rate, staircase=False, name=None):
        def f(gs):
            return torch.tensor(float(exponential_decay_value(learning_rate, gs, decay_steps, decay_rate, staircase)),
                                dtype=tf_shim.float_dtype())
        return T(f, [global_step])

    class ScheduledAdam(tf_shim._Adam):
        """AdamOptimizer whose learning_rate may be a graph node, read at each step; minimize(global_step=...) adds 1
        to the variable after the update (optimizer.py:apply_gradients)"""

        def __init__(self, learning_rate=0.001, **kw):
            tf_shim._Adam.__init__(self, learning_rate, **kw)
            self.node, self.global_step, self.rates = learning_rate, None, []

        def minimize(self, loss, global_step=None, var_list=None, name=None):
            self.global_step = global_step
            return tf_shim._Minimize(self, loss)

        def begin(self, dt):
            if isinstance(self.node, T):
                with torch.no_grad():
                    self.lr = float(tf_shim._evaluate([self.node], {})[0])
            self.rates.append(self.lr)
            tf_shim._Adam.begin(self, dt)

        def finish(self):
            tf_shim._Adam.finish(self)
            if self.global_step is not None:
                self.global_step.value = self.global_step.value + 1

    def matmul(a, b, transpose_a=False, transpose_b=False, name=None):
        """math_ops.matmul on batches of matrices: the transposes swap the LAST two dimensions"""
        def f(x, y):
            x = x.transpose(-1, -2) if transpose_a else x
            y = y.transpose(-1, -2) if transpose_b else y
            return x @ y
        return T(f, [a, b])

    tf_shim.gather_nd, tf_shim.to_int32, tf_shim.matmul = gather_nd, to_int32, matmul
    tf_shim.nn.sparse_softmax_cross_entropy_with_logits = sparse_softmax_cross_entropy_with_logits
    tf_shim.nn.dynamic_rnn = dynamic_rnn
    tf_shim.train.exponential_decay = exponential_decay
    tf_shim.train.AdamOptimizer = ScheduledAdam
    tf_shim.zeros_initializer = lambda dtype=None: (lambda shape, dtype=None, partition_info=None:
                                                    np.zeros([int(s) for s in shape], np.float32))
    return check_srgnn_ops()


def check_srgnn_ops():
    """every attached op on a small hand-computed value"""
    tf = tf_shim
    run = lambda t: tf._evaluate([t], {})[0]
    tf.set_float("float64")
    tf.reset_default_graph()
    tf._GRAPH.collections = {}
    G.CELLS.clear()
    m = tf.constant(np.asarray([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]))
    assert run(tf.gather_nd(m, tf.constant(np.asarray([[0, 2], [1, 0], [1, 1]])))).tolist() == [3.0, 4.0, 5.0]
    cube = tf.constant(np.arange(8.0).reshape(2, 2, 2))
    assert run(tf.gather_nd(cube, tf.constant(np.asarray([[1, 0], [0, 1]])))).tolist() == [[4.0, 5.0], [2.0, 3.0]]
    # logits [0, log 3]: softmax = [1/4, 3/4]; the large row must not overflow: the maximum is subtracted
    z = tf.constant(np.asarray([[0.0, np.log(3.0)], [1000.0, 0.0]]))
    ce = run(tf.nn.sparse_softmax_cross_entropy_with_logits(labels=tf.constant(np.asarray([0, 1])), logits=z))
    assert abs(float(ce[0]) - np.log(4.0)) < 1e-15 and float(ce[1]) == 1000.0
    assert run(tf.to_int32(tf.constant(np.asarray([2.0, 2.9, -1.5])))).tolist() == [2, 2, -1]
    assert run(tf.stack([tf.range(2), tf.to_int32(tf.constant(np.asarray([3.0, 1.0]))) - 1], axis=1)).tolist() == \
        [[0, 2], [1, 0]]
    # one step of the cell: n = 1, in = 1 (the value make_golden_gru4rec.attach_ops checks), through dynamic_rnn
    cell = tf.nn.rnn_cell.GRUCell(1)
    out, h = tf.nn.dynamic_rnn(cell, tf.constant(np.asarray([[[1.0]]])), initial_state=tf.constant(np.asarray([[0.5]])))
    for var, val in zip(cell.vars, ([[0.5, 0.5], [0.5, 0.5]], [0.0, 0.0], [[0.5], [0.5]], [0.0])):
        var.load(np.asarray(val))
    g = 1.0 / (1.0 + np.exp(-0.75))
    want = g * 0.5 + (1 - g) * np.tanh(0.5 * 1.0 + 0.5 * (g * 0.5))
    assert abs(float(run(h)) - want) < 1e-15 and run(out).tolist() == [[[float(run(h))]]]
    # staircase: 0.5 * 0.1 ^ floor(step / 2.5) in float32; continuous at step 5 of 10: 0.5 * 0.1 ^ 0.5
    gs = tf.Variable(0)
    lr = tf.train.exponential_decay(0.5, global_step=gs, decay_steps=2.5, decay_rate=0.1, staircase=True)
    seen = []
    for k in range(6):
        gs.load(np.asarray(k))
        seen.append(float(run(lr)))
    f32 = np.float32
    assert seen[:5] == [float(f32(0.5))] * 3 + [float(f32(0.5) * f32(0.1))] * 2 and abs(seen[5] - 0.005) < 1e-9, seen
    gs.load(np.asarray(5))
    cont = float(run(tf.train.exponential_decay(0.5, gs, 10, 0.1)))
    assert abs(cont - 0.5 * 0.1 ** 0.5) < 1e-7
    # Adam on f(w) = w^2 / 2 at w = 1 with rate 0.5 0.1^floor(step / 1): the first step moves by lr, the second by 0.1 lr
    gs.load(np.asarray(0))
    w = tf.Variable(np.asarray([1.0]))
    opt = tf.train.AdamOptimizer(tf.train.exponential_decay(0.5, gs, 1, 0.1, staircase=True))
    mz = opt.minimize(tf.reduce_sum(w * w) / 2.0, global_step=gs)
    sess = tf.Session(seed=0)
    _, loss = sess.run([mz, mz.loss])
    # m = 0.1 g, v = 0.001 g^2, lr_t = 0.5 sqrt(0.001) / 0.1: the step is 0.5 sqrt(v) / (sqrt(v) + eps)
    w1, e = float(w.value), 1 - 0.999
    assert loss == 0.5 and int(gs.value) == 1 and abs(w1 - (1.0 - 0.5 * np.sqrt(e) / (np.sqrt(e) + 1e-8))) < 1e-12
    sess.run(mz)
    step2 = w1 - float(w.value)
    m2, v2 = 0.1 + (w1 - 0.1) * (1 - 0.9), e + (w1 * w1 - e) * e
    want2 = float(f32(0.5) * f32(0.1)) * np.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2) * m2 / (np.sqrt(v2) + 1e-8)
    assert int(gs.value) == 2 and opt.rates == [0.5, float(f32(0.5) * f32(0.1))] and abs(step2 - want2) < 1e-12, \
        (step2, want2)
    zv = tf.get_variable("z", [3], dtype=tf.float32, initializer=tf.zeros_initializer())
    assert zv.numpy().tolist() == [0.0, 0.0, 0.0]
    m3 = tf.matmul(tf.constant(np.asarray([[[1.0, 2.0]]])), tf.constant(np.asarray([[[3.0, 4.0], [5.0, 6.0]]])),
                   transpose_b=True)
    assert run(m3).tolist() == [[[11.0, 17.0]]]
    G.CELLS.clear()
    tf._GRAPH.collections = {}
    tf.reset_default_graph()
    return True


class FeedSession(G.RecordingSession):
    """the recording session; the feeds are kept by placeholder identity (SRGNN.py's placeholders have no names)"""

    def __init__(self, *a, **k):
        G.RecordingSession.__init__(self, *a, **k)
        self.id_log = None

    def run(self, fetches, feed_dict=None):
        if self.id_log is not None and feed_dict is not None:
            self.id_log.append({id(k): v for k, v in feed_dict.items()})
        return G.RecordingSession.run(self, fetches, feed_dict)


def build(dataset, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    tf_shim._GRAPH.collections = {}
    G.CELLS.clear()
    mod = load_srgnn()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "SRGNN"
    conf.update(hyper)
    sess = FeedSession(seed=0)
    model = mod.SRGNN(sess, dataset, conf)
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess


def _hyper(case, batch, n_samples):
    d, step, nonhybrid, l2, L, lr_dc = P.CASES[case]
    # decay_steps = lr_dc_step n_samples / batch_size: 2 steps at B_STEP in `hybrid`, far away in the others
    lr_dc_step = 2.0 * B_STEP / n_samples if case == "hybrid" else 3
    return dict(lr=P.LR, L2=l2, hidden_size=d, step=step, batch_size=batch, epochs=1, lr_dc=lr_dc, lr_dc_step=lr_dc_step,
                nonhybrid=nonhybrid, max_seq_len=L, topk=20)


def _variables(d):
    variables = list(tf_shim._GRAPH.variables)
    assert len(variables) == len(P.NAMES) + 1 and variables[-1].value.dtype.is_floating_point is False
    for v, name in zip(variables, P.NAMES):
        assert tuple(v.value.shape) == P.shapes(131, d)[name], (name, v.value.shape)
    return variables[:len(P.NAMES)]


def _load(variables, init):
    for var, n in zip(variables, P.NAMES):
        var.load(init[n])


def _tabs(variables):
    return [v.numpy() for v in variables]


def count_samples(seqs):
    return sum(max(len(s) - 1, 0) for s in seqs.values())


def repeats_dict(I, L, seed):
    """a hand-made train dict whose sessions repeat items: the five named patterns first, then seeded walks over small
    item pools"""
    rs = np.random.RandomState(seed)
    seqs = {0: [5, 5, 7, 3, 9],                              # a consecutive repeat: a self-loop
            1: [1, 2, 1, 2, 3, 8],                           # the edge 1 -> 2 taken twice
            2: [9, 4],                                       # a session of one item
            3: [6, 6, 6, 6, 2],                              # a session of one item repeated
            4: [int(x) for x in rs.randint(0, 30, L + 2)]}   # sessions at the full length
    for u in range(5, 40):
        pool = rs.choice(I, rs.randint(2, 7), replace=False)
        seqs[u] = [int(x) for x in rs.choice(pool, rs.randint(2, 16))]
    return seqs


def make_batches(model, case, L, seed):
    """STEPS batches of B_STEP sample indices; in `repeats` every batch holds the five named patterns"""
    rs = np.random.RandomState(seed)
    n = len(model.train_seq)
    out = []
    for s in range(STEPS):
        rows = []
        if case == "repeats":
            kinds = {"consecutive": lambda q: len(set(q)) > 1 and any(a == b for a, b in zip(q, q[1:])),
                     "twice": lambda q: len(set(zip(q, q[1:]))) < len(q) - 1 and len(set(q)) > 1,
                     "one": lambda q: len(q) == 1,
                     "one repeated": lambda q: len(q) > 1 and len(set(q)) == 1,
                     "full": lambda q: len(q) == L}
            for name, test in kinds.items():
                hits = [k for k in range(n) if test(list(model.train_seq[k])) and k not in rows]
                assert hits, name
                rows.append(hits[s % len(hits)])
        rest = np.setdiff1d(np.arange(n), rows)
        rows += rs.choice(rest, B_STEP - len(rows), replace=False).tolist()
        out.append(np.asarray(rows)[rs.permutation(B_STEP)])
    return out


def padded(sessions, L, I):
    out = np.full((len(sessions), L), I, np.int32)
    for k, q in enumerate(sessions):
        assert 1 <= len(q) <= L
        out[k, :len(q)] = q
    return out


def run_case(ds, case, init, batches, n_samples, with_predict=None):
    d, step, nonhybrid, l2, L, _ = P.CASES[case]
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, _hyper(case, B_STEP, n_samples), width)
        assert len(model.train_seq) == n_samples
        variables = _variables(d)
        _load(variables, init)
        tabs, losses, feeds = [], [], []
        for rows in batches:
            sessions = [model.train_seq[k] for k in rows]
            tars = [model.train_tar[k] for k in rows]
            adj_in, adj_out, alias, items, mask = model._build_session_graph(sessions)
            feed = {model.target_ph: tars, model.item_ph: items, model.adj_in_ph: adj_in, model.adj_out_ph: adj_out,
                    model.alias_ph: alias, model.mask_ph: mask}
            _, loss = sess.run([model.train_opt, model.train_opt.loss], feed_dict=feed)
            losses.append(float(loss))
            tabs.append(_tabs(variables))
            feeds.append(dict(seq=padded(sessions, L, 131), target=np.asarray(tars, np.int32),
                              adj_in=np.asarray(adj_in, np.float64), adj_out=np.asarray(adj_out, np.float64),
                              alias=np.asarray(alias, np.int32), items=np.asarray(items, np.int32),
                              mask=np.asarray(mask, np.int32)))
        out[tag] = (tabs, losses, feeds, list(model.train_opt.opt.rates))
        if with_predict is not None:
            users, cand = with_predict
            out[tag + "_predict"] = _np(model.predict(list(users), None), width)
            out[tag + "_predict_cand"] = _np(model.predict(list(users), [list(c) for c in cand]), width)
    return out


def pack_tables(case, tabs_by_tag, init):
    """the f64 trace as differences from the initial values.  The vectors (biases, nasrv: some start at zero, so the
    difference is the whole value) as float32, exact to 2^-24 of the difference.  The matrices as int16 counts of each
    step's own scale max|difference| / 32767 — float32 differences would take the file past the size limit (hidden_size
    72 has 88,000 values per step).  Their round trip is within max|difference| / 65000 and, asserted here, within 1e-6
    max|value|: a tenth of the 1e-5 max|want| that reads it, spent out of the device's margin, not added to it.  Of the
    f32 twin only what the tests read: its distance from the f64 trace per step and variable"""
    out = {}
    for j, name in enumerate(P.NAMES):
        i64 = init[name].astype(np.float64)
        want = np.stack([t[j] for t in tabs_by_tag["f64"]]).astype(np.float64)
        delta = want - i64[None]
        if min(init[name].shape) == 1 or init[name].ndim == 1:
            back = i64[None] + delta.astype(np.float32).astype(np.float64)
            assert np.abs(back - want).max(initial=0) <= 2.0 ** -24 * np.abs(delta).max(initial=0)
            out["%s_f64_%s" % (case, name)] = delta.astype(np.float32)
        else:
            scale = np.abs(delta).reshape(len(delta), -1).max(axis=1) / 32767.0
            safe = np.where(scale > 0, scale, 1.0).reshape((-1,) + (1,) * (delta.ndim - 1))
            q = np.rint(delta / safe).astype(np.int16)
            back = i64[None] + q.astype(np.float64) * safe
            lost = np.abs(back - want).reshape(len(want), -1).max(axis=1)
            assert (lost <= np.abs(delta).reshape(len(want), -1).max(axis=1) / 65000.0).all()
            assert (lost <= 1e-6 * np.abs(want).reshape(len(want), -1).max(axis=1)).all(), name
            out["%s_q_%s" % (case, name)] = q
            out["%s_scale_%s" % (case, name)] = np.where(scale > 0, scale, 1.0)
        twin = np.stack([t[j] for t in tabs_by_tag["f32"]]).astype(np.float64)
        out["%s_gap_%s" % (case, name)] = np.abs(twin - want).reshape(len(want), -1).max(axis=1)
    return out


def run_epoch(ds, init, n_samples):
    d = P.CASES["hybrid"][0]
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, _hyper("hybrid", B_EPOCH, n_samples), width)
        variables = _variables(d)
        _load(variables, init)
        order = []
        inner = model._shuffle_index

        def recording(seq_index, inner=inner, order=order):
            for bat in inner(seq_index):
                order.append([int(k) for k in bat])
                yield bat
        model._shuffle_index = recording
        np.random.seed(EPOCH_SEED)
        sess.id_log = []
        model.train_model()
        fed = [f for f in sess.id_log if id(model.target_ph) in f]
        sess.id_log = None
        assert len(fed) == len(order)
        for f, bat in zip(fed, order):                        # the session saw those samples, in that order
            assert list(f[id(model.target_ph)]) == [model.train_tar[k] for k in bat]
        out[tag] = dict(order=np.asarray(order, np.int64), tabs=[_tabs(variables)],
                        rates=list(model.train_opt.opt.rates), train_seq=model.train_seq, train_tar=model.train_tar,
                        train=model.user_pos_train)
    assert np.array_equal(out["f32"]["order"], out["f64"]["order"]) and out["f32"]["rates"] == out["f64"]["rates"]
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_srgnn_ops()
    from neurec_amd.model.sequential_recommender.SRGNN import train_samples
    R = toy_matrix(isolated=False)
    U, I = R.shape
    seqs = time_orders(R)
    ds = TimedDataset(R, seqs)
    ptr = np.zeros(U + 1, np.int64)
    for u, s in seqs.items():
        ptr[u + 1] = len(s)
    ptr = np.cumsum(ptr)
    rep = repeats_dict(I, P.CASES["repeats"][4], seed=99)
    rep_ds = TimedDataset(R, rep)
    rep_ptr = np.zeros(U + 1, np.int64)
    for u, s in rep.items():
        rep_ptr[u + 1] = len(s)
    rep_ptr = np.cumsum(rep_ptr)
    out = dict(shape=np.asarray(R.shape, np.int64), seq_ptr=ptr,
               seq=np.asarray([i for u in sorted(seqs) for i in seqs[u]], np.int32), rep_ptr=rep_ptr,
               rep=np.asarray([i for u in sorted(rep) for i in rep[u]], np.int32), lr=np.float64(P.LR),
               cases=np.asarray(sorted(P.CASES)), batch_step=np.int64(B_STEP), batch_epoch=np.int64(B_EPOCH))
    lens = np.diff(ptr)
    present = [u for u in np.argsort(-lens, kind="stable") if lens[u] > 0]
    predict_users = np.asarray(present[:9] + present[-9:] + present[40:49], np.int32)
    assert len(predict_users) == N_PREDICT and N_PREDICT % B_STEP
    rs = np.random.RandomState(7)
    cand = rs.randint(0, I, (N_PREDICT, 3)).astype(np.int32)
    cand[0] = [3, 0, I - 1]
    out.update(predict_users=predict_users, predict_cand=cand)
    gaps = {}
    for k, case in enumerate(sorted(P.CASES)):
        d, step, nonhybrid, l2, L, _ = P.CASES[case]
        data, train = (rep_ds, rep) if case == "repeats" else (ds, seqs)
        n_samples = count_samples(train)
        init = P.init_tables(I, d, seed=800 + k)
        model, _ = build(data, _hyper(case, B_STEP, n_samples), "float64")
        batches = make_batches(model, case, L, FEED_SEED + k)
        last = case == P.PREDICT_CASE
        res = run_case(data, case, init, batches, n_samples, (predict_users, cand) if last else None)
        out["%s_init_seed" % case] = np.int64(800 + k)
        feeds = res["f64"][2]
        out["%s_seq" % case] = np.stack([f["seq"] for f in feeds])
        out["%s_target" % case] = np.stack([f["target"] for f in feeds])
        for s, f in enumerate(feeds):
            assert all(np.array_equal(f[nm], res["f32"][2][s][nm]) for nm in f)
            for nm in ("adj_in", "adj_out", "alias", "items", "mask"):
                out["%s_%d_%s" % (case, s, nm)] = f[nm]
        assert res["f32"][3] == res["f64"][3]
        out["%s_lrs" % case] = np.asarray(res["f64"][3], np.float32)
        assert np.array_equal(out["%s_lrs" % case].astype(np.float64), np.asarray(res["f64"][3]))
        for tag, _ in WIDTHS:
            out["%s_loss_%s" % (case, tag)] = np.asarray(res[tag][1], np.float64)
        out.update(pack_tables(case, {tag: res[tag][0] for tag, _ in WIDTHS}, init))
        if last:
            for tag, _ in WIDTHS:
                out["predict_" + tag] = res[tag + "_predict"]
                out["predict_cand_" + tag] = res[tag + "_predict_cand"]
        gaps[case] = max(out["%s_gap_%s" % (case, t)].max() for t in P.NAMES)
    lrs = out["hybrid_lrs"]
    assert lrs[0] == lrs[1] and lrs[2] == lrs[3] and lrs[2] < 0.11 * lrs[0], lrs       # the rate drops before step 3
    assert not out["gated_q_B"].any()                                                 # nonhybrid at L2 = 0
    # one whole epoch of train_model()
    d = P.CASES["hybrid"][0]
    n_samples = count_samples(seqs)
    init = P.init_tables(I, d, seed=890)
    ep = run_epoch(ds, init, n_samples)
    order = ep["f64"]["order"]
    users, ends, lengths = train_samples(ep["f64"]["train"], P.CASES["hybrid"][4])
    for k in range(n_samples):                                # the plugin's samples are the class's, index by index
        row = ep["f64"]["train"][int(users[k])]
        L = P.CASES["hybrid"][4]
        assert list(row[max(0, ends[k] - L):ends[k]]) == list(ep["f64"]["train_seq"][k])
        assert row[ends[k]] == ep["f64"]["train_tar"][k] and lengths[k] == len(ep["f64"]["train_seq"][k])
    out["epoch_init_seed"] = np.int64(890)
    out.update(epoch_order=order, epoch_users=users[order], epoch_ends=ends[order],
               epoch_lrs=np.asarray(ep["f64"]["rates"], np.float32), epoch_seed=np.int64(EPOCH_SEED),
               epoch_lr_dc_step=np.float64(_hyper("hybrid", B_EPOCH, n_samples)["lr_dc_step"]))
    out.update(pack_tables("epoch", {tag: ep[tag]["tabs"] for tag, _ in WIDTHS}, init))
    gaps["epoch"] = max(out["epoch_gap_%s" % t].max() for t in P.NAMES)
    path = os.path.join(HERE, "tfgraph_srgnn.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); %d epoch steps; fp32 vs fp64 table gaps %s; predict gap %.3g" % (
        path, os.path.getsize(path), len(order), {k: "%.3g" % v for k, v in gaps.items()},
        np.abs(out["predict_f32"] - out["predict_f64"]).max()))


if __name__ == "__main__":
    main()
