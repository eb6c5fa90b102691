"""Golden GRU4Rec trace produced by the REFERENCE's own GRU4Rec class (model/sequential_recommender/GRU4Rec.py).

The class is loaded whole and unchanged with oracle/ref_models._load_file and runs under oracle/tf_shim.py, as
make_golden_transrec.py does for TransRec.  Ops of GRU4Rec.py the shim lacks are attached from here (attach_ops), each
checked on a small hand-computed value.  The ONE piece of this trace that TensorFlow itself does not pin is the
restated GRUCell [EXT: tensorflow r1.12 rnn_cell_impl.GRUCell]: gates = sigmoid([x, s] Wg + bg) split r first, u second;
c = act([x, r * s] Wc + bc); h = u s + (1 - u) c — written here from its published definition, its variables made
through the shim's Variable so that the optimiser sees them as dense.

    python tests/golden/make_golden_gru4rec.py              # needs the reference tree

Writes tests/golden/tfgraph_gru4rec.npz:
  indptr / indices / shape     the train pattern: toy_matrix(isolated=False) (157 x 131)
  seq_ptr / seq                every user's items by time: a seeded permutation of the row
  data_uit / offset_idx        as GRU4Rec._init_data builds them
  <case>_init_<var>            the initial variables of the case (float32), <var> of gru4rec_restatement.table_names
  <case>_X / _Y / _reset       the batches [steps, B] and the slots zeroed after each step
  <case>_rows_{E_in,Q,b}       the rows of that table that differ from their initial value at any step, in either width
  <case>_{f32,f64}_<var>       [steps, ...]: those rows (the cells' variables: whole) after each step MINUS their
                               initial value, in float64
  <case>_{f32,f64}_state<l>    [steps, B, n_l]: the fetched final_state of each step (before the reset)
  epoch_*                      one train_model() epoch at batch_size 16 with a recording session: epoch_perm, epoch_X /
                               epoch_Y [S, 16], epoch_zero [S, 16] (state rows all zero on entry), the end tables as
                               above under the case name `epoch`
  user_emb_{f32,f64}           _get_user_embeddings() after the last step of the case `top1_tanh_linear`
  predict_users, predict_{f32,f64}, predict_cand, predict_cand_{f32,f64}   predict() there, full and candidate mode
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
import gru4rec_restatement as P               # noqa: E402

B_STEP, B_EPOCH, STEPS = 20, 16, 3
EPOCH_SEED = 4242
RESETS = {0: (1, 7), 1: (0, 7, 19)}          # step -> the slots zeroed after it

_SHADOWED = ("util", "util.tool", "util.learner", "data", "evaluator", "model", "model.AbstractRecommender",
             "model.sequential_recommender")
CELLS = []                                    # the GRUCell instances of the graph being built, in creation order


def load_gru4rec():
    """the reference module model/sequential_recommender/GRU4Rec.py, executed under the shim"""
    saved_tf = tf_shim.install()
    saved = {k: sys.modules.get(k) for k in _SHADOWED}
    try:
        tool = rm._load_file("util.tool", os.path.join(rm.REF, "util", "tool.py"))
        learner = rm._load_file("util.learner", os.path.join(rm.REF, "util", "learner.py"))
        util = types.ModuleType("util")
        util.__path__ = []
        util.tool, util.learner = tool, learner
        for fn in ("timer", "l2_loss", "inner_product", "log_loss", "csr_to_user_dict", "csr_to_user_dict_bytime"):
            setattr(util, fn, getattr(tool, fn))
        util.Logger = rm.MemoryLogger
        sys.modules["util"] = util
        data = types.ModuleType("data")
        sys.modules["data"] = data
        ev = types.ModuleType("evaluator")
        ev.ProxyEvaluator = rm.RecordingEvaluator
        sys.modules["evaluator"] = ev
        model_pkg = types.ModuleType("model")
        model_pkg.__path__ = []
        sys.modules["model"] = model_pkg
        rm._load_file("model.AbstractRecommender", os.path.join(rm.REF, "model", "AbstractRecommender.py"))
        mod = rm._load_file("model.sequential_recommender.GRU4Rec",
                            os.path.join(rm.REF, "model", "sequential_recommender", "GRU4Rec.py"))
        sys.modules.pop("model.sequential_recommender.GRU4Rec", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


class GRUCell:
    """[EXT: tensorflow r1.12 rnn_cell_impl.GRUCell] restated: variables gates/kernel [in + n, 2 n], gates/bias [2 n]
    (ones), candidate/kernel [in + n, n], candidate/bias [n] (zeros), made at the first call as TF's build() does"""

    def __init__(self, num_units, activation=None, **_):
        self.n, self.act = int(num_units), activation or tf_shim.tanh
        self.vars = None
        CELLS.append(self)

    def _build(self, n_in):
        n, k = self.n, CELLS.index(self)
        rs = np.random.RandomState(11 + k)

        def glorot(rows, cols):
            lim = np.sqrt(6.0 / (rows + cols))
            return rs.uniform(-lim, lim, (rows, cols)).astype(np.float32)
        self.vars = (tf_shim.Variable(glorot(n_in + n, 2 * n), name="gru%d/gates/kernel" % k),
                     tf_shim.Variable(np.ones(2 * n, np.float32), name="gru%d/gates/bias" % k),
                     tf_shim.Variable(glorot(n_in + n, n), name="gru%d/candidate/kernel" % k),
                     tf_shim.Variable(np.zeros(n, np.float32), name="gru%d/candidate/bias" % k))

    def __call__(self, inputs, state, n_in):
        if self.vars is None:
            self._build(n_in)
        Wg, bg, Wc, bc = self.vars
        n = self.n
        gates = tf_shim.sigmoid(tf_shim.matmul(tf_shim.concat([inputs, state], 1), Wg) + bg)
        r, u = gates[:, :n], gates[:, n:]
        c = self.act(tf_shim.matmul(tf_shim.concat([inputs, r * state], 1), Wc) + bc)
        h = u * state + (1 - u) * c
        return h, h


class DropoutWrapper:
    """rnn_cell_impl.DropoutWrapper with its default arguments (every keep probability 1.0): the identity"""

    def __init__(self, cell, **kw):
        assert not kw, kw
        self.cell = cell

    def __call__(self, inputs, state, n_in):
        return self.cell(inputs, state, n_in)


class MultiRNNCell:
    """rnn_cell_impl.MultiRNNCell: layer l takes its own state from the list and feeds its output to layer l + 1"""

    def __init__(self, cells):
        self.cells = list(cells)

    def __call__(self, inputs, state):
        assert len(state) == len(self.cells)
        cur, new = inputs, []
        n_in = int(cur.inputs[0].value.shape[1])              # the looked-up table's width
        for cell, s in zip(self.cells, state):
            cur, ns = cell(cur, s, n_in)
            new.append(ns)
            n_in = cell.cell.n if isinstance(cell, DropoutWrapper) else cell.n
        return cur, tuple(new)


def attach_ops():
    """ops of GRU4Rec.py the shim lacks, by their published definitions, each checked here on a small value"""
    import torch

    def reshape(tensor, shape, name=None):
        return tf_shim.Tensor(lambda a: a.reshape(*[int(s) for s in shape]), [tensor])

    def matrix_diag_part(input, name=None):                 # noqa: A002
        return tf_shim.Tensor(lambda a: torch.diagonal(a, dim1=-2, dim2=-1), [input])

    def gather(params, indices, name=None, **_):
        return tf_shim.nn.embedding_lookup(params, indices)   # the shim's gather kind: a sparse update for `b`

    def truncated_normal(shape, mean=0.0, stddev=1.0, dtype=None, seed=None, name=None):
        """values beyond two standard deviations are redrawn; the makers overwrite the variables afterwards"""
        rs = np.random.RandomState(2017)

        def f():
            a = rs.randn(*[int(s) for s in shape])
            while (np.abs(a) > 2).any():
                bad = np.abs(a) > 2
                a[bad] = rs.randn(int(bad.sum()))
            return tf_shim._to_torch((mean + stddev * a).astype(np.float32))
        return tf_shim.Tensor(f, [])

    tf_shim.reshape, tf_shim.matrix_diag_part, tf_shim.gather = reshape, matrix_diag_part, gather
    tf_shim.random = types.SimpleNamespace(truncated_normal=truncated_normal)
    tf_shim.nn.rnn_cell = types.SimpleNamespace(GRUCell=GRUCell, DropoutWrapper=DropoutWrapper,
                                                MultiRNNCell=MultiRNNCell)
    run = lambda t: tf_shim._evaluate([t], {})[0]
    tf_shim.set_float("float64")
    x = tf_shim.constant(np.asarray([[1.0, 2.0], [3.0, 4.0]]))
    assert run(matrix_diag_part(x)).tolist() == [1.0, 4.0]
    assert run(reshape(matrix_diag_part(x), shape=[-1, 1])).tolist() == [[1.0], [4.0]]
    v = tf_shim.Variable(np.asarray([5.0, 6.0, 7.0]))
    gth = gather(v, tf_shim.constant(np.asarray([2, 0, 2])))
    assert gth.kind == "gather" and run(gth).tolist() == [7.0, 5.0, 7.0]
    tn = run(truncated_normal([50, 4], stddev=0.01))
    assert tuple(tn.shape) == (50, 4) and float(tn.abs().max()) <= 0.02 + 1e-9
    # the cell on a hand-computed value: n = 1, in = 1, x = 1, s = 0.5, every weight 0.5, gate bias 0, tanh
    CELLS.clear()
    cell = GRUCell(1, activation=tf_shim.tanh)
    h, _ = cell(tf_shim.constant(np.asarray([[1.0]])), tf_shim.constant(np.asarray([[0.5]])), 1)
    for var, val in zip(cell.vars, ([[0.5, 0.5], [0.5, 0.5]], [0.0, 0.0], [[0.5], [0.5]], [0.0])):
        var.load(np.asarray(val))
    g = 1.0 / (1.0 + np.exp(-0.75))                          # r = u = sigmoid(0.5 * 1 + 0.5 * 0.5)
    want = g * 0.5 + (1 - g) * np.tanh(0.5 * 1.0 + 0.5 * (g * 0.5))
    assert abs(float(run(h)) - want) < 1e-15, (float(run(h)), want)
    CELLS.clear()
    tf_shim.reset_default_graph()
    for name in ("pow", "sigmoid", "squeeze", "reduce_mean", "identity", "zeros", "log_sigmoid"):
        assert hasattr(tf_shim, name), name
    return True


class RecordingSession(tf_shim.Session):
    """the shim's Session with fetch lists that hold tuples (`[update_opt, final_state]`), and a log of the feeds"""

    def __init__(self, *a, **k):
        tf_shim.Session.__init__(self, *a, **k)
        self.feed_log = None

    def run(self, fetches, feed_dict=None):
        if self.feed_log is not None and feed_dict is not None:
            self.feed_log.append({getattr(k, "name", None): np.array(v) for k, v in feed_dict.items()})
        if not isinstance(fetches, (list, tuple)):
            return tf_shim.Session.run(self, fetches, feed_dict)
        flat, shape = [], []
        for f in fetches:
            if isinstance(f, (list, tuple)):
                shape.append(len(f))
                flat.extend(f)
            else:
                shape.append(None)
                flat.append(f)
        vals = tf_shim.Session.run(self, flat, feed_dict)
        out, k = [], 0
        for n in shape:
            if n is None:
                out.append(vals[k])
                k += 1
            else:
                out.append(list(vals[k:k + n]))
                k += n
        return out


def build(dataset, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    CELLS.clear()
    mod = load_gru4rec()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "GRU4Rec"
    conf.update(hyper)
    sess = RecordingSession(seed=0)
    model = mod.GRU4Rec(sess, dataset, conf)
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess


def _variables(model):
    out = [model.input_embeddings, model.item_embeddings, model.item_biases]
    for cell in CELLS:
        out += list(cell.vars)
    return out


def make_batches(n_items, steps, B, seed):
    """X and Y hold duplicates, one item is an input and an output of the same step, the hub item 0 takes part"""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        X, Y = rs.randint(1, n_items, B), rs.randint(1, n_items, B)
        X[1], Y[3], Y[4], X[6], Y[7] = X[0], Y[2], X[5], 0, 0
        assert len(set(X.tolist())) < B and len(set(Y.tolist())) < B and set(X.tolist()) & set(Y.tolist())
        out.append((X.astype(np.int32), Y.astype(np.int32)))
    return out


def run_case(ds, init, hyper, batches, with_predict=None):
    out = {}
    L = len(hyper["layers"])
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, hyper, width)
        variables = _variables(model)
        assert len(variables) == len(init)
        for var, t in zip(variables, init):
            var.load(t)
        dt = np.float32 if width == "float32" else np.float64
        state = [np.zeros((len(batches[0][0]), n), dt) for n in hyper["layers"]]
        tabs, states = [], []
        for k, (X, Y) in enumerate(batches):
            feed = {model.X_ph: X, model.Y_ph: Y}
            for l in range(L):
                feed[model.state_ph[l]] = state[l]
            _, state = sess.run([model.update_opt, model.final_state], feed_dict=feed)
            state = [np.array(s, dt) for s in state]
            states.append([s.copy() for s in state])
            tabs.append([v.numpy() for v in variables])
            for l in range(L):
                state[l][list(RESETS.get(k, ()))] = 0
        out[tag] = (tabs, states)
        if with_predict is not None:
            users, cand = with_predict
            model.evaluate_model()
            out[tag + "_user_emb"] = _np(model.cur_user_embeddings, width)
            out[tag + "_predict"] = _np(model.predict(list(users), None), width)
            out[tag + "_predict_cand"] = _np(model.predict(list(users), [list(c) for c in cand]), width)
    return out


def pack_tables(case, names, tabs_by_tag, init):
    """rows that moved (E_in, Q, b) or the whole variable (the cells'), as the DIFFERENCE from the initial value in
    float64 (make_golden_transrec.pack)"""
    out = {}
    init64 = [t.astype(np.float64) for t in init]
    for j, name in enumerate(names):
        if name in ("E_in", "Q", "b"):
            moved = np.zeros(len(init[j]), bool)
            for tabs in tabs_by_tag.values():
                for t in tabs:
                    diff = t[j].astype(np.float64) != init64[j]
                    moved |= diff.reshape(len(diff), -1).any(axis=1)
            rows = np.flatnonzero(moved).astype(np.int32)
            out["%s_rows_%s" % (case, name)] = rows
        else:
            rows = slice(None)
        for tag, width in WIDTHS:
            tabs = tabs_by_tag[tag]
            delta = np.stack([t[j].astype(np.float64)[rows] - init64[j][rows] for t in tabs])
            back = (init64[j][rows][None] + delta).astype(np.float32 if width == "float32" else np.float64)
            want = np.stack([t[j][rows] for t in tabs])
            assert np.array_equal(back, want) if width == "float32" else np.abs(back - want).max(initial=0) < 1e-15
            out["%s_%s_%s" % (case, tag, name)] = delta
    return out


def run_epoch(ds, init, hyper):
    """train_model() for one epoch; the session records every feed"""
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, hyper, width)
        variables = _variables(model)
        for var, t in zip(variables, init):
            var.load(t)
        np.random.seed(EPOCH_SEED)
        perm = np.random.permutation(len(model.offset_idx) - 1)
        np.random.seed(EPOCH_SEED)
        sess.feed_log = []
        model.train_model()
        feeds = [f for f in sess.feed_log if "output" in f]          # the training feeds carry Y_ph
        sess.feed_log = None
        X = np.stack([f["input"] for f in feeds]).astype(np.int32)
        Y = np.stack([f["output"] for f in feeds]).astype(np.int32)
        zero = np.stack([(f["layer_0_state"] == 0).all(axis=1) for f in feeds])
        out[tag] = dict(perm=perm, X=X, Y=Y, zero=zero, tabs=[[v.numpy() for v in variables]])
    a, b = out["f32"], out["f64"]
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["zero"], b["zero"]) and np.array_equal(a["perm"], b["perm"])
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_ops()
    R = toy_matrix(isolated=False)
    U, I = R.shape
    seqs = time_orders(R)
    assert len(seqs) == U
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
    predict_users = np.asarray([order[0], order[1], order[len(order) // 2], order[-1], 3], np.int32)
    cand = np.asarray([[3, 0, I - 1], [7, 7, 1], [0, 1, 2], [I - 1, I - 2, 5], [9, 8, 0]], np.int32)
    out.update(predict_users=predict_users, predict_cand=cand)
    gaps = {}
    for k, case in enumerate(sorted(P.CASES)):
        loss, hact, fact, layers, reg = P.CASES[case]
        hyper = dict(lr=P.LR, reg=reg, layers=list(layers), batch_size=B_STEP, loss=loss, hidden_act=hact,
                     final_act=fact, epochs=1, topk=20)
        names = P.table_names(len(layers))
        tables = P.init_tables(I, layers, seed=900 + k)
        init = [tables[n] for n in names]
        batches = make_batches(I, STEPS, B_STEP, seed=700 + k)
        last = case == P.PREDICT_CASE
        res = run_case(ds, init, hyper, batches, (predict_users, cand) if last else None)
        for n, t in zip(names, init):
            out["%s_init_%s" % (case, n)] = t
        out[case + "_X"] = np.stack([b[0] for b in batches])
        out[case + "_Y"] = np.stack([b[1] for b in batches])
        reset = np.zeros((STEPS, B_STEP), bool)
        for s, slots in RESETS.items():
            reset[s, list(slots)] = True
        out[case + "_reset"] = reset
        out.update(pack_tables(case, names, {tag: res[tag][0] for tag, _ in WIDTHS}, init))
        for tag, _ in WIDTHS:
            for l in range(len(layers)):
                out["%s_%s_state%d" % (case, tag, l)] = np.stack([st[l] for st in res[tag][1]]).astype(np.float64)
        if last:
            for tag, _ in WIDTHS:
                out["user_emb_" + tag] = res[tag + "_user_emb"]
                out["predict_" + tag] = res[tag + "_predict"]
                out["predict_cand_" + tag] = res[tag + "_predict_cand"]
        gaps[case] = max(np.abs(out["%s_f32_%s" % (case, t)] - out["%s_f64_%s" % (case, t)]).max() for t in names)
    # _init_data as the class builds it, and one whole epoch
    loss, hact, fact, layers, reg = P.CASES[P.PREDICT_CASE]
    hyper = dict(lr=P.LR, reg=reg, layers=list(layers), batch_size=B_EPOCH, loss=loss, hidden_act=hact, final_act=fact,
                 epochs=1, topk=20)
    model, _ = build(ds, hyper, "float64")
    out["data_uit"], out["offset_idx"] = model.data_uit.astype(np.int32), model.offset_idx.astype(np.int32)
    names = P.table_names(len(layers))
    tables = P.init_tables(I, layers, seed=990)
    init = [tables[n] for n in names]
    ep = run_epoch(ds, init, hyper)
    for n, t in zip(names, init):
        out["epoch_init_%s" % n] = t
    out.update(epoch_perm=ep["f64"]["perm"].astype(np.int64), epoch_X=ep["f64"]["X"], epoch_Y=ep["f64"]["Y"],
               epoch_zero=ep["f64"]["zero"], epoch_seed=np.int64(EPOCH_SEED))
    out.update(pack_tables("epoch", names, {tag: ep[tag]["tabs"] for tag, _ in WIDTHS}, init))
    gaps["epoch"] = max(np.abs(out["epoch_f32_%s" % t] - out["epoch_f64_%s" % t]).max() for t in names)
    path = os.path.join(HERE, "tfgraph_gru4rec.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); %d epoch steps; fp32 vs fp64 table gaps %s; user_emb gap %.3g; predict gap %.3g" % (
        path, os.path.getsize(path), len(out["epoch_X"]), {k: "%.3g" % v for k, v in gaps.items()},
        np.abs(out["user_emb_f32"] - out["user_emb_f64"]).max(), np.abs(out["predict_f32"] - out["predict_f64"]).max()))


if __name__ == "__main__":
    main()
