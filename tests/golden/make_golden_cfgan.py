"""Golden CFGAN trace produced by the REFERENCE's own class (model/general_recommender/CFGAN.py).

The class is loaded whole and unchanged (make_golden_neumf.load_class) and run under oracle/tf_shim.py.  The ops it needs
beyond the shim's are attached here by their published definitions [EXT: tensorflow r1.12] and put on small hand-computed
values by check_ops() before use; nothing under oracle/ changes:
  layers.Dense       kernel [in, units] and a zero bias, created at the first apply() under the layer's name;
                     activation(x kernel + bias)
  GraphKeys, get_collection
                     the trainable variables whose name starts with the scope
  ones_like, zeros_like
  Optimizer.minimize(loss, var_list=...)
                     honours its list (the shim's own ignores it): d loss / d listed variable only, every optimiser
                     object with its own slots and beta powers
`util.tool` (randint_choice, csr_to_user_dict, l2_loss) and `util.data_iterator` are the reference's own files.  The class
runs its own train_model(): the masks come from its get_train_data() and the batches from its two DataIterators, both on
numpy's global stream, seeded here; an iterator subclass and the session only WRITE DOWN what passes through them.

    python tests/golden/make_golden_cfgan.py              # needs the reference tree

Writes tests/golden/tfgraph_cfgan.npz.  Every case (cfgan_restatement.CASES) is one train_model() of two outer epochs:
  shape, indptr, indices       the train matrix, 27 users x 131 items: user 5 has no train item, item 3 is held by two
                               users in three
  <case>_init_seed             the initial variables are cfgan_restatement.init_tables(n_cols, G, D, seed)
  <case>_kinds                 one letter per step in the order run: d = sess.run(trainer_d), g = sess.run(trainer_g)
  <case>_rows [S, Bmax], <case>_sizes [S]
                               the batch of each step (rows of R: users, or items in itemBased), filled up with -1
  <case>_zr, <case>_pm [S, Bmax, words]
                               the fed masks as bit rows, column 32 w + k at bit k of word w (zr of a d step: zeros)
  <case>_f64_<var> [S1, ...]   the variable after each step of the FIRST outer epoch (S1 steps), float64 run, MINUS its
                               initial value; <case>_gap_<var> [S1]: max |float32 run - float64 run| after each step
  <case>_end_<var>, <case>_endgap_<var>
                               the same after the last step of the second outer epoch
  <case>_ratings_{f32,f64}     all_ratings_for_test [27, 131] after the last step (cases user and item)
  <case>_log                   the lines train_model() logged
"""
import os
import sys
import types

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_models as rm          # noqa: E402
from oracle import tf_shim                    # noqa: E402
from make_golden_tfgraph import WIDTHS, _np, _reset_recorders   # noqa: E402
import make_golden_neumf as N                 # noqa: E402
import cfgan_restatement as P                 # noqa: E402

N_USERS, N_ITEMS = 27, 131
RATINGS_CASES = ("user", "item")


def train_matrix():
    """27 x 131: user 5 empty, item 3 with two users in three, one long row"""
    rs = np.random.RandomState(2018)
    dense = rs.random_sample((N_USERS, N_ITEMS)) < 0.07
    dense[:, 3] = np.arange(N_USERS) % 3 != 0
    dense[11, :] = rs.random_sample(N_ITEMS) < 0.6
    dense[5, :] = False
    m = sp.csr_matrix(dense.astype(np.float32))
    m.sort_indices()
    return m


# ------------------------------------------------------------------ the ops CFGAN.py needs beyond the shim's
def _width(t):
    """the static last dimension of a node: a Dense output, a concat, a placeholder, or what an elementwise op's inputs
    have"""
    if getattr(t, "_width", None) is not None:
        return t._width
    if t.kind == "placeholder":
        return int(t.shape[-1])
    found = [w for w in (_width(i) for i in t.inputs) if w is not None]
    return max(found) if found else None


class _MinimizeListed(tf_shim._Minimize):
    """minimize(loss, var_list=...): only the listed variables are differentiated and moved"""

    def __init__(self, opt, loss, var_list):
        tf_shim._Minimize.__init__(self, opt, loss)
        listed = {id(v) for v in var_list}
        assert listed <= {id(v) for v in self.vars}, "a listed variable is not reached by the loss"
        self.vars = [v for v in self.vars if id(v) in listed]
        self.state = {id(v): self.state[id(v)] for v in self.vars}


def attach_cfgan_ops():
    import torch
    T = tf_shim.Tensor
    shim_concat = tf_shim.concat
    if getattr(shim_concat, "cfgan", False):
        return

    class Dense:
        def __init__(self, units, activation=None, kernel_initializer=None, name=None, **_):
            self.units, self.activation, self.init, self.name = int(units), activation, kernel_initializer, name
            self.kernel = self.bias = None

        def apply(self, x):
            if self.kernel is None:
                n_in = _width(x)
                assert n_in is not None, "Dense %s: the input's width is unknown" % self.name
                self.kernel = tf_shim.Variable(self.init([n_in, self.units]), name="%s/kernel" % self.name)
                self.bias = tf_shim.Variable(np.zeros(self.units, np.float32), name="%s/bias" % self.name)
            y = tf_shim.add(tf_shim.matmul(x, self.kernel), self.bias)
            y = y if self.activation is None else self.activation(y)
            y._width = self.units
            return y
        __call__ = apply

    def concat(values, axis, name=None):
        out = shim_concat(values, axis, name)
        if axis in (1, -1):
            out._width = sum(_width(v) for v in values)
        return out
    concat.cfgan = True

    def get_collection(key, scope=None):
        assert key == "trainable_variables"
        return [v for v in tf_shim._GRAPH.variables if v.trainable and (scope is None or (v.name or "").startswith(scope))]

    def ones_like(x, dtype=None, name=None):
        return T(lambda a: torch.ones_like(a), [x])

    def zeros_like(x, dtype=None, name=None):
        return T(lambda a: torch.zeros_like(a), [x])

    def minimize(self, loss, global_step=None, var_list=None, name=None):
        return tf_shim._Minimize(self, loss) if var_list is None else _MinimizeListed(self, loss, list(var_list))

    tf_shim.layers = types.SimpleNamespace(Dense=Dense)
    tf_shim.GraphKeys = types.SimpleNamespace(TRAINABLE_VARIABLES="trainable_variables")
    tf_shim.concat, tf_shim.get_collection = concat, get_collection
    tf_shim.ones_like, tf_shim.zeros_like = ones_like, zeros_like
    tf_shim._Optimizer.minimize = minimize
    return check_ops()


def check_ops():
    """every attached op on a small hand-computed value"""
    tf = tf_shim
    tf.set_float("float64")
    tf.reset_default_graph()
    sess = tf.Session(seed=0)
    x = tf.placeholder(tf.float32, [None, 2])
    const = lambda a: (lambda shape, dtype=None, partition_info=None: np.asarray(a, np.float32))   # noqa: E731
    la = tf.layers.Dense(2, activation=tf.identity, kernel_initializer=const([[1.0, 2.0], [3.0, 4.0]]), name="aa_h0")
    lb = tf.layers.Dense(1, activation=tf.sigmoid, kernel_initializer=const([[1.0], [-1.0], [0.5], [0.0]]), name="bb_out")
    h = la.apply(x)
    y = lb.apply(tf.concat([x, h], 1))
    feed = {x: np.asarray([[1.0, 1.0]])}
    assert sess.run(h, feed).tolist() == [[4.0, 6.0]]                      # [1, 1] [[1, 2], [3, 4]] + 0
    assert abs(float(sess.run(y, feed)[0, 0]) - 1.0 / (1.0 + np.exp(-2.0))) < 1e-15    # 1 - 1 + 0.5 4 + 0 = 2
    names = [v.name for v in tf._GRAPH.variables]
    assert names == ["aa_h0/kernel", "aa_h0/bias", "bb_out/kernel", "bb_out/bias"], names
    a_vars = tf.get_collection(tf.GraphKeys.TRAINABLE_VARIABLES, scope="aa")
    b_vars = tf.get_collection(tf.GraphKeys.TRAINABLE_VARIABLES, scope="bb")
    assert [v.name for v in a_vars] == names[:2] and [v.name for v in b_vars] == names[2:]
    assert sess.run(tf.ones_like(h), feed).tolist() == [[1.0, 1.0]] and sess.run(tf.zeros_like(y), feed).tolist() == [[0.0]]
    # two optimisers over one loss, disjoint lists: each moves its own variables only, and only on its own runs.
    # loss = sum(h) = x . kernel columns + bias: d / d kernel = [[1, 1], [1, 1]], d / d bias = [1, 1]
    loss = tf.reduce_sum(h) + tf.reduce_sum(y)
    op_a = tf.train.GradientDescentOptimizer(0.5).minimize(loss, var_list=a_vars[1:])      # the bias alone
    op_b = tf.train.AdamOptimizer(0.1).minimize(loss, var_list=b_vars)
    before = [v.numpy() for v in tf._GRAPH.variables]
    sess.run(op_a, feed)
    after = [v.numpy() for v in tf._GRAPH.variables]
    dy = 1.0 / (1.0 + np.exp(-2.0)) * (1.0 - 1.0 / (1.0 + np.exp(-2.0)))   # through y: bias_a . [0.5, 0] of bb's kernel
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2]) and np.array_equal(after[3], before[3])
    assert np.allclose(after[1], before[1] - 0.5 * np.asarray([1.0 + 0.5 * dy, 1.0]), atol=1e-15)
    sess.run(op_b, feed)
    last = [v.numpy() for v in tf._GRAPH.variables]
    assert np.array_equal(last[0], after[0]) and np.array_equal(last[1], after[1])
    assert not np.array_equal(last[2], after[2]) and not np.array_equal(last[3], after[3])
    assert op_a.opt is not op_b.opt and float(op_b.opt.b1p) == 0.9 * 0.9    # Adam's powers moved once, by its own run
    assert set(op_b.state) == {id(v) for v in b_vars} and set(op_a.state) == {id(a_vars[1])}
    tf.reset_default_graph()
    return True


# ------------------------------------------------------------------ the class, with recorders around it
class RecordingSession(tf_shim.Session):
    """the shim's Session; every run of a minimisation is written down: which trainer, the fed masks, the variables
    afterwards"""

    def __init__(self, *a, **k):
        tf_shim.Session.__init__(self, *a, **k)
        self.model, self.steps = None, []

    def run(self, fetches, feed_dict=None):
        out = tf_shim.Session.run(self, fetches, feed_dict)
        m = self.model
        if m is not None and isinstance(fetches, tf_shim._Minimize):
            kind = "d" if fetches is m.trainer_d else "g"
            assert kind == "d" or fetches is m.trainer_g
            assert np.array_equal(feed_dict[m.condition], feed_dict[m.real_data])
            self.steps.append(dict(kind=kind, cond=np.asarray(feed_dict[m.condition]), pm=np.asarray(feed_dict[m.mask]),
                                   zr=np.asarray(feed_dict[m.g_zr_dims]) if kind == "g" else None,
                                   tabs=[v.numpy() for v in tf_shim._GRAPH.variables]))
        return out


def recording_iterator(base, log):
    class Recording(base):
        def __iter__(self):
            for batch in base.__iter__(self):
                log.append(np.asarray(batch, np.int64))
                yield batch
    return Recording


def hyper_of(case):
    mode, hg, hd, reg_g, reg_d, opt_g, opt_d, step_d, step_g = P.CASES[case]
    return dict(epochs=2 * step_g, mode=mode, reg_G=reg_g, reg_D=reg_d, lr_G=P.LR_G, lr_D=P.LR_D, batchSize_G=P.BATCH_G,
                batchSize_D=P.BATCH_D, opt_G=opt_g, opt_D=opt_d, hiddenLayer_G=list(hg), hiddenLayer_D=list(hd),
                step_G=step_g, step_D=step_d, ZR_ratio=P.ZR_RATIO, ZP_ratio=P.ZP_RATIO, ZR_coefficient=P.ZR_COEF, verbose=1)


def run_case(ds, case, init, seed):
    mode, hg, hd = P.CASES[case][:3]
    n_rows, n_cols = ds.train_matrix.shape[::-1] if mode == "itemBased" else ds.train_matrix.shape
    R = (ds.train_matrix.T if mode == "itemBased" else ds.train_matrix).tocsr()
    dense = np.asarray(R.todense())
    want_names = P.names(len(hg), len(hd))
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        tf_shim.set_float(width)
        tf_shim.reset_default_graph()
        mod = N.load_class("CFGAN")
        conf = rm.Conf(rm.NEUREC_DEFAULTS)
        conf["recommender"] = "CFGAN"
        conf.update(hyper_of(case))
        sess = RecordingSession(seed=0)
        model = mod.CFGAN(sess, ds, conf)
        model.build_graph()
        sess.run(tf_shim.global_variables_initializer())
        variables = list(tf_shim._GRAPH.variables)
        got_names = [v.name.replace("/", "_") for v in variables]
        assert got_names == want_names, got_names
        shapes = P.shapes(n_cols, hg, hd)
        assert [tuple(v.value.shape) for v in variables] == [shapes[n] for n in want_names]
        for var, n in zip(variables, want_names):
            var.load(init[n])
        batches = []
        mod.DataIterator = recording_iterator(mod.DataIterator, batches)
        sess.model = model
        np.random.seed(seed)
        model.train_model()
        steps = sess.steps
        assert len(steps) == len(batches)
        for st, rows in zip(steps, batches):
            assert np.array_equal(st["cond"], dense[rows]), "a fed batch is not the rows the iterator gave"
            pos = dense[rows] > 0
            for plane in ("pm", "zr"):
                if st[plane] is not None:
                    m = st[plane] > 0
                    assert set(np.unique(st[plane])) <= {0.0, 1.0}
                    assert (m[pos.any(1)] >= pos[pos.any(1)]).all() and not m[~pos.any(1)].any()
        out[tag] = dict(steps=steps, batches=batches, log=list(rm.MemoryLogger.lines),
                        ratings=_np(model.all_ratings_for_test, width))
    a, b = out["f32"], out["f64"]
    assert len(a["steps"]) == len(b["steps"]) and a["log"] == b["log"]
    for sa, sb, ra, rb in zip(a["steps"], b["steps"], a["batches"], b["batches"]):
        assert sa["kind"] == sb["kind"] and np.array_equal(ra, rb) and np.array_equal(sa["pm"], sb["pm"])
        assert (sa["zr"] is None) == (sb["zr"] is None) and (sa["zr"] is None or np.array_equal(sa["zr"], sb["zr"]))
    return out, want_names, n_cols


def pack(case, res, names, init, n_cols):
    steps, batches = res["f64"]["steps"], res["f64"]["batches"]
    S, bmax, words = len(steps), max(len(b) for b in batches), (n_cols + 31) // 32
    kinds = "".join(st["kind"] for st in steps)
    assert S % 2 == 0 and kinds[:S // 2] == kinds[S // 2:]
    S1 = S // 2
    rows = np.full((S, bmax), -1, np.int32)
    zr, pm = (np.zeros((S, bmax, words), np.uint32) for _ in range(2))
    for s, (st, b) in enumerate(zip(steps, batches)):
        rows[s, :len(b)] = b
        pm[s, :len(b)] = P.to_bits(st["pm"])
        if st["zr"] is not None:
            zr[s, :len(b)] = P.to_bits(st["zr"])
    out = {"%s_kinds" % case: np.asarray(kinds), "%s_rows" % case: rows,
           "%s_sizes" % case: np.asarray([len(b) for b in batches], np.int64), "%s_zr" % case: zr, "%s_pm" % case: pm,
           "%s_log" % case: np.asarray(res["f64"]["log"])}
    for j, name in enumerate(names):
        want = np.stack([st["tabs"][j] for st in steps]).astype(np.float64)
        twin = np.stack([st["tabs"][j] for st in res["f32"]["steps"]]).astype(np.float64)
        gap = np.abs(twin - want).reshape(S, -1).max(axis=1, initial=0)
        delta = want - init[name].astype(np.float64)[None]
        out["%s_f64_%s" % (case, name)] = delta[:S1]
        out["%s_gap_%s" % (case, name)] = gap[:S1]
        out["%s_end_%s" % (case, name)] = delta[-1]
        out["%s_endgap_%s" % (case, name)] = gap[-1]
    if case in RATINGS_CASES:
        out["%s_ratings_f32" % case] = res["f32"]["ratings"].astype(np.float32)
        out["%s_ratings_f64" % case] = res["f64"]["ratings"].astype(np.float64)
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_cfgan_ops()
    Rm = train_matrix()
    assert Rm.shape == (N_USERS, N_ITEMS) and Rm.indptr[6] == Rm.indptr[5] and Rm[:, 3].nnz >= 16
    ds = rm.Dataset(Rm)
    out = dict(shape=np.asarray(Rm.shape, np.int64), indptr=Rm.indptr.astype(np.int64), indices=Rm.indices.astype(np.int32),
               cases=np.asarray(sorted(P.CASES)))
    gaps = {}
    for k, case in enumerate(sorted(P.CASES)):
        mode, hg, hd = P.CASES[case][:3]
        n_cols = N_USERS if mode == "itemBased" else N_ITEMS
        init = P.init_tables(n_cols, hg, hd, seed=1300 + k)
        res, names, n_cols = run_case(ds, case, init, seed=7600 + k)
        out["%s_init_seed" % case] = np.int64(1300 + k)
        out.update(pack(case, res, names, init, n_cols))
        gaps[case] = max(out["%s_gap_%s" % (case, n)].max(initial=0) for n in names)
        # a batch must hold item 3 (userBased) more than once, and the empty row
        if mode == "userBased":
            rows = out["%s_rows" % case]
            assert any((Rm[r[r >= 0]][:, 3].nnz > 1) for r in rows) and any(5 in r for r in rows)
    path = os.path.join(HERE, "tfgraph_cfgan.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); steps %s; fp32 vs fp64 table gaps %s" % (
        path, os.path.getsize(path), {c: len(str(out["%s_kinds" % c])) for c in sorted(P.CASES)},
        {k: "%.3g" % v for k, v in gaps.items()}))


if __name__ == "__main__":
    main()
