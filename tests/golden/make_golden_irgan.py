"""Golden IRGAN trace produced by the REFERENCE's own class (model/general_recommender/IRGAN.py).

The class is loaded whole and unchanged (make_golden_neumf.load_class) and run under oracle/tf_shim.py.  What the shim
lacks is attached here by its published definition [EXT: tensorflow r1.12] and put on small hand-computed values by
check_ops() before use; nothing under oracle/ changes:
  gather(params, ids)   array_ops.gather on axis 0 (the shim's embedding_lookup: a variable all of whose consumers are
                        gathers gets the sparse update)
  reshape(x, shape)
  variable_scope        the shim has it (a name scope)
  Optimizer.minimize(loss, var_list=...)
                        honours its list (make_golden_cfgan._MinimizeListed) and SUMS a vector loss first: TensorFlow's
                        grad_ys default to ones, the shim's autograd.grad needs a scalar
The surroundings of the class that are inputs, not computation, are stood in for: `dataset.trainMatrix` is the train CSR;
the thread pool of get_train_data() maps in order (its `np.random.choice` calls share one global stream, so their order
under real threads is not defined); `np.random.choice` is numpy's own in the float64 run and WRITTEN DOWN, and the float32
run is handed the float64 run's draws (numpy's is still called, so that the global stream the DataIterator shuffles from
moves the same way): both widths then walk the same steps, and their distance is rounding alone.  The initial G goes
through a pickle in a temporary directory, read by the class's own build_graph().

    python tests/golden/make_golden_irgan.py              # needs the reference tree

Writes tests/golden/tfgraph_irgan.npz.  Every case (irgan_restatement.CASES) is one train_model() of two epochs:
  shape, indptr, indices        the train matrix, 23 users x 67 items: user 4 has no train item, user 9 only item 0,
                                user 2 item 0 and others, user 13 one item (17), user 11 a long row
  <case>_init_seed              the initial tables are irgan_restatement.init_tables(23, 67, 5, seed)
  <case>_kinds                  one letter per step in the order run: d = sess.run(d_updates), g = sess.run(gan_updates)
  <case>_pass_ptr [n_d + 1], <case>_pass_users / _items / _labels, <case>_pass_order
                                every D pass's triples as get_train_data() returned them and the shuffled index order
                                its DataIterator walked (batches of 8, the last one short)
  <case>_d_users / _d_items / _d_labels [n_d steps, 8], <case>_d_sizes
                                the fed batch of every D step, filled up with -1
  <case>_g_user [n_g steps], <case>_g_samples [n_g steps, Smax], <case>_g_sizes
                                the user and the 2 deg samples of every G step, filled up with -1
  <case>_f64_<table> [steps of the table's network in the FIRST epoch, ...]
                                the table after each of those steps, float64 run, MINUS its initial value;
                                <case>_gap_<table>: max |float32 run - float64 run| after each
  <case>_end_<table>, <case>_endgap_<table>
                                the same after the last step of the second epoch
  <case>_ratings_{f32,f64}      predict(all users, None) at the last evaluate()
  <case>_log                    the lines train_model() logged
"""
import os
import pickle
import sys
import tempfile

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_models as rm          # noqa: E402
from oracle import tf_shim                    # noqa: E402
from make_golden_tfgraph import _reset_recorders   # noqa: E402
from make_golden_cfgan import _MinimizeListed  # noqa: E402
import make_golden_neumf as N                 # noqa: E402
import irgan_restatement as P                 # noqa: E402

N_USERS, N_ITEMS = 23, 67


def train_matrix():
    rs = np.random.RandomState(2019)
    dense = rs.random_sample((N_USERS, N_ITEMS)) < 0.035
    dense[:, 0] = False
    for u in range(N_USERS):                                   # nobody empty by accident
        if not dense[u].any():
            dense[u, 1 + (7 * u) % (N_ITEMS - 1)] = True
    dense[4, :] = False                                        # no train item
    dense[9, :] = False
    dense[9, 0] = True                                         # item 0 alone: any([0]) is False
    dense[2, 0] = True                                         # item 0 and others
    dense[2, 30] = True
    dense[13, :] = False
    dense[13, 17] = True                                       # degree 1
    dense[11, :] = rs.random_sample(N_ITEMS) < 0.5             # a long row
    m = sp.csr_matrix(dense.astype(np.float32))
    m.sort_indices()
    return m


# ------------------------------------------------------------------ the ops IRGAN.py needs beyond the shim's
def attach_irgan_ops():
    T = tf_shim.Tensor
    if getattr(tf_shim, "irgan_ops", False):
        return True

    def gather(params, indices, name=None, **_):
        return tf_shim.nn.embedding_lookup(params, indices)

    def reshape(tensor, shape, name=None):
        return T(lambda a: a.reshape(tuple(int(s) for s in shape)), [tensor])

    def minimize(self, loss, global_step=None, var_list=None, name=None):
        total = tf_shim.reduce_sum(loss)
        return tf_shim._Minimize(self, total) if var_list is None else _MinimizeListed(self, total, list(var_list))

    tf_shim.gather, tf_shim.reshape = gather, reshape
    tf_shim._Optimizer.minimize = minimize
    tf_shim.irgan_ops = True
    return check_ops()


def check_ops():
    """every attached op on a small hand-computed value"""
    tf = tf_shim
    tf.set_float("float64")
    tf.reset_default_graph()
    sess = tf.Session(seed=0)
    with tf.variable_scope("scope"):
        v = tf.Variable(np.asarray([1.0, 2.0, 4.0]))
    ids = tf.placeholder(tf.int32)
    assert sess.run(tf.gather(v, ids), {ids: [2, 0, 2]}).tolist() == [4.0, 1.0, 4.0]
    assert float(sess.run(tf.gather(v, ids), {ids: 1})) == 2.0
    m = tf.reshape(tf.constant(np.arange(6.0)), [1, -1])
    assert sess.run(m).shape == (1, 6) and sess.run(tf.reshape(m, [-1])).tolist() == list(range(6))
    # a vector loss [2 v_2, 3 v_0, 5 v_2] + (v_0 + v_1 + v_2): its sum is differentiated, so the scalar counts 3 times:
    # d / d v = [3 + 3, 3, 2 + 5 + 3] = [6, 3, 10]
    loss = tf.gather(v, ids) * tf.constant(np.asarray([2.0, 3.0, 5.0])) + tf.reduce_sum(v)
    op = tf.train.GradientDescentOptimizer(0.5).minimize(loss, var_list=[v])
    sess.run(op, {ids: [2, 0, 2]})
    assert np.allclose(v.numpy(), [1.0 - 3.0, 2.0 - 1.5, 4.0 - 5.0], atol=1e-15), v.numpy()
    # a variable reached through gathers only moves on the gathered rows
    w = tf.Variable(np.asarray([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]]))
    op2 = tf.train.GradientDescentOptimizer(1.0).minimize(
        tf.reduce_sum(tf.nn.embedding_lookup(w, ids), 1), var_list=[w])
    sess.run(op2, {ids: [1, 1]})
    assert w.numpy().tolist() == [[1.0, 1.0], [0.0, 0.0], [3.0, 3.0]]
    tf.reset_default_graph()
    return True


# ------------------------------------------------------------------ the class, with recorders around it
class _SerialPool:
    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def map(self, fn, it):
        return [fn(x) for x in it]


class _Random:
    """np.random as the class sees it: choice() written down, or replayed while numpy's own still runs"""

    def __init__(self, replay=None):
        self.log, self.replay, self.at = [], replay, 0

    def choice(self, a, size=None, p=None):
        got = np.random.choice(a, size=size, p=p)
        if self.replay is not None:
            got = self.replay[self.at].copy()
            assert len(got) == size
            self.at += 1
        self.log.append(np.asarray(got).copy())
        return got

    def __getattr__(self, attr):
        return getattr(np.random, attr)


class _Numpy:
    def __init__(self, random):
        self.random = random

    def __getattr__(self, attr):
        return getattr(np, attr)


class RecordingSession(tf_shim.Session):
    def __init__(self, *a, **k):
        tf_shim.Session.__init__(self, *a, **k)
        self.model, self.steps = None, []

    def run(self, fetches, feed_dict=None):
        out = tf_shim.Session.run(self, fetches, feed_dict)
        m = self.model
        if m is not None and isinstance(fetches, tf_shim._Minimize):
            g, d = m.generator, m.discriminator
            tabs = [v.numpy() for v in g.g_params + d.d_params]
            if fetches is d.d_updates:
                self.steps.append(dict(kind="d", users=np.asarray(feed_dict[d.u]), items=np.asarray(feed_dict[d.i]),
                                       labels=np.asarray(feed_dict[d.label]), tabs=tabs))
            else:
                assert fetches is g.gan_updates
                self.steps.append(dict(kind="g", user=int(feed_dict[g.u]), samples=np.asarray(feed_dict[g.i]),
                                       reward=np.asarray(feed_dict[g.reward]), tabs=tabs))
        return out


def recording_iterator(base, log):
    class Recording(base):
        def __iter__(self):
            order = []
            log.append(order)
            for idx in self.batch_sampler:
                order.extend(idx)
                yield [list(s) for s in zip(*[self.dataset[i] for i in idx])]
    return Recording


def run_case(ds, case, init, seed, tmp):
    g_reg, d_reg, d_tau, d_epoch, g_epoch = P.CASES[case]
    path = os.path.join(tmp, "%s.pkl" % case)
    with open(path, "wb") as f:
        pickle.dump([init["g_P"], init["g_Q"], init["g_b"]], f)
    out, draws = {}, None
    for tag, width in (("f64", "float64"), ("f32", "float32")):
        _reset_recorders()
        rm.RecordingEvaluator.users = list(range(N_USERS))
        tf_shim.set_float(width)
        tf_shim.reset_default_graph()
        mod = N.load_class("IRGAN")
        conf = rm.Conf(rm.NEUREC_DEFAULTS)
        conf["recommender"] = "IRGAN"
        conf.update(dict(factors_num=P.FACTORS, lr=P.LR, g_reg=g_reg, d_reg=d_reg, epochs=2, g_epoch=g_epoch,
                         d_epoch=d_epoch, batch_size=P.BATCH, d_tau=d_tau, pretrain_file=path))
        sess = RecordingSession(seed=0)
        model = mod.IRGAN(sess, ds, conf)
        assert sorted(model.user_pos_train) == P.train_users(ds.train_matrix.indptr, ds.train_matrix.indices)
        tf_shim._RUN["session"] = sess                          # D's random_uniform initial values are drawn at creation
        try:
            model.build_graph()
        finally:
            tf_shim._RUN["session"] = None
        sess.run(tf_shim.global_variables_initializer())
        variables = model.generator.g_params + model.discriminator.d_params
        assert [tuple(v.value.shape) for v in variables] == [init[n].shape for n in P.NAMES]
        for var, n in zip(variables[:3], P.NAMES):
            assert np.array_equal(var.numpy().astype(np.float32), init[n])          # the pickle came through
        for var, n in zip(variables, P.NAMES):
            var.load(init[n])
        orders, passes = [], []
        rnd = _Random(draws)
        mod.np = _Numpy(rnd)
        mod.ThreadPoolExecutor = _SerialPool
        mod.DataIterator = recording_iterator(mod.DataIterator, orders)
        inner = model.get_train_data

        def get_train_data():
            data = inner()
            passes.append(tuple(np.asarray(x) for x in data))
            return data
        model.get_train_data = get_train_data
        sess.model = model
        np.random.seed(seed)
        model.train_model()
        if draws is None:
            draws = rnd.log
        ratings = np.asarray(rm.RecordingEvaluator.ratings[-1])
        out[tag] = dict(steps=sess.steps, orders=[np.asarray(o, np.int64) for o in orders], passes=passes,
                        log=list(rm.MemoryLogger.lines), ratings=ratings)
    a, b = out["f32"], out["f64"]
    assert len(a["steps"]) == len(b["steps"]) and a["log"][2:] == b["log"][2:]
    for sa, sb in zip(a["steps"], b["steps"]):
        assert sa["kind"] == sb["kind"]
        for k in ("users", "items", "labels", "samples"):
            assert k not in sa or np.array_equal(sa[k], sb[k])
        assert sa.get("user") == sb.get("user")
    return out


def pack(case, res, init):
    steps, orders, passes = res["f64"]["steps"], res["f64"]["orders"], res["f64"]["passes"]
    g_reg, d_reg, d_tau, d_epoch, g_epoch = P.CASES[case]
    kinds = "".join(st["kind"] for st in steps)
    S = len(steps)
    assert S % 2 == 0 and kinds[:S // 2] == kinds[S // 2:] and len(orders) == len(passes) == 2 * d_epoch
    S1 = S // 2
    d_steps = [st for st in steps if st["kind"] == "d"]
    g_steps = [st for st in steps if st["kind"] == "g"]
    out = {"%s_kinds" % case: np.asarray(kinds), "%s_log" % case: np.asarray(res["f64"]["log"])}
    ptr = np.concatenate([[0], np.cumsum([len(p[0]) for p in passes])]).astype(np.int64)
    out["%s_pass_ptr" % case] = ptr
    out["%s_pass_users" % case] = np.concatenate([p[0] for p in passes]).astype(np.int32)
    out["%s_pass_items" % case] = np.concatenate([p[1] for p in passes]).astype(np.int32)
    out["%s_pass_labels" % case] = np.concatenate([p[2] for p in passes]).astype(np.float32)
    out["%s_pass_order" % case] = np.concatenate(orders).astype(np.int32)
    assert all(sorted(o.tolist()) == list(range(len(p[0]))) for o, p in zip(orders, passes))
    du, di = (np.full((len(d_steps), P.BATCH), -1, np.int32) for _ in range(2))
    dl = np.full((len(d_steps), P.BATCH), -1, np.float32)
    for s, st in enumerate(d_steps):
        n = len(st["users"])
        du[s, :n], di[s, :n], dl[s, :n] = st["users"], st["items"], st["labels"]
    out.update({"%s_d_users" % case: du, "%s_d_items" % case: di, "%s_d_labels" % case: dl,
                "%s_d_sizes" % case: np.asarray([len(st["users"]) for st in d_steps], np.int64)})
    smax = max(len(st["samples"]) for st in g_steps)
    gs = np.full((len(g_steps), smax), -1, np.int32)
    for s, st in enumerate(g_steps):
        gs[s, :len(st["samples"])] = st["samples"]
    out.update({"%s_g_user" % case: np.asarray([st["user"] for st in g_steps], np.int32), "%s_g_samples" % case: gs,
                "%s_g_sizes" % case: np.asarray([len(st["samples"]) for st in g_steps], np.int64)})
    for j, name in enumerate(P.NAMES):
        kind = name[0]
        which = [s for s in range(S) if kinds[s] == kind]
        want = np.stack([steps[s]["tabs"][j] for s in which]).astype(np.float64)
        twin = np.stack([res["f32"]["steps"][s]["tabs"][j] for s in which]).astype(np.float64)
        gap = np.abs(twin - want).reshape(len(which), -1).max(axis=1)
        delta = want - init[name].astype(np.float64)[None]
        first = sum(1 for s in which if s < S1)
        out["%s_f64_%s" % (case, name)] = delta[:first]
        out["%s_gap_%s" % (case, name)] = gap[:first]
        out["%s_end_%s" % (case, name)] = steps[-1]["tabs"][j].astype(np.float64) - init[name].astype(np.float64)
        out["%s_endgap_%s" % (case, name)] = np.abs(res["f32"]["steps"][-1]["tabs"][j].astype(np.float64) -
                                                     steps[-1]["tabs"][j].astype(np.float64)).max()
        # the network that did not step is bit-unchanged by the step
        for s in range(1, S):
            if kinds[s] != kind:
                assert np.array_equal(steps[s]["tabs"][j], steps[s - 1]["tabs"][j]), (case, s, name)
    out["%s_ratings_f32" % case] = res["f32"]["ratings"].astype(np.float32)
    out["%s_ratings_f64" % case] = res["f64"]["ratings"].astype(np.float64)
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_irgan_ops()
    Rm = train_matrix()
    deg = np.diff(Rm.indptr)
    assert Rm.shape == (N_USERS, N_ITEMS) and deg[4] == 0 and Rm[9].indices.tolist() == [0] and deg[13] == 1
    assert Rm[2].indices[0] == 0 and deg[2] > 1 and deg[11] >= 20
    ds = rm.Dataset(Rm)
    ds.trainMatrix = ds.train_matrix                            # IRGAN.py:128 reads the older attribute name
    out = dict(shape=np.asarray(Rm.shape, np.int64), indptr=Rm.indptr.astype(np.int64), indices=Rm.indices.astype(np.int32),
               cases=np.asarray(sorted(P.CASES)))
    gaps = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, case in enumerate(sorted(P.CASES)):
            init = P.init_tables(N_USERS, N_ITEMS, P.FACTORS, seed=2300 + k)
            res = run_case(ds, case, init, seed=8600 + k, tmp=tmp)
            out["%s_init_seed" % case] = np.int64(2300 + k)
            out.update(pack(case, res, init))
            gaps[case] = max(out["%s_gap_%s" % (case, n)].max(initial=0) for n in P.NAMES)
    path = os.path.join(HERE, "tfgraph_irgan.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); nnz %d; steps %s; fp32 vs fp64 table gaps %s" % (
        path, os.path.getsize(path), Rm.nnz, {c: len(str(out["%s_kinds" % c])) for c in sorted(P.CASES)},
        {k: "%.3g" % v for k, v in gaps.items()}))


if __name__ == "__main__":
    main()
