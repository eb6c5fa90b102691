"""Golden TransRec trace produced by the REFERENCE's own TransRec class (model/sequential_recommender/TransRec.py).

The class is loaded whole and unchanged with oracle/ref_models._load_file and runs under oracle/tf_shim.py, as
make_golden_fpmc.py does for FPMC: the same stand-ins (`util` re-exporting the reference's tool / learner functions,
`data` with replay samplers under the names TransRec.py imports, `evaluator`, `model`), plus the reference's own
util/data_iterator.py, which predict() uses.  The maker drives `sess.run((model.loss, model.optimizer), feed_dict)`
itself; train_model() is not called.  predict() is the reference's.

    python tests/golden/make_golden_transrec.py              # needs the reference tree

Writes tests/golden/tfgraph_transrec.npz:
  indptr / indices / shape     the train pattern: toy_matrix() (157 x 131)
  seq_ptr / seq                every user's items by time: a seeded permutation of the row
  P_0 / Q_0 / b_0 / T_0        the initial tables (0.1 randn; b [I], T [1, d]); hyper-parameters as scalars
  <case>_users/_recent/_items/_third   the batches [steps, B] (third = labels, or the negatives in the pairwise cases)
  <case>_reg_mf                the case's regulariser weight
  <case>_rows_{P,Q,b}          the rows of that table that differ from its initial value at any step, in either width —
                               every other row equals its initial value after every step
  <case>_{f32,f64}_{P,Q,b}     [steps, len(rows), ...]: those rows after each step MINUS their initial value, in
                               float64; <case>_{f32,f64}_T [steps, 1, d]: T whole, likewise;
                               <case>_{f32,f64}_loss [steps]: the fetched (pre-update) loss
  predict_users, predict_{f32,f64}, predict_cand, predict_cand_{f32,f64}
                               predict() rows after the last step of the case `ce_adam`, full and candidate mode
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
import transrec_restatement as P              # noqa: E402

HYPER = dict(epochs=1, batch_size=64, embedding_size=16, reg_mf=P.REG, learning_rate=0.01, learner="adam",
             is_pairwise=False, num_neg=4, loss_function="cross_entropy", init_method="normal", stddev=0.01, verbose=1,
             topk=20)
STEPS = {"ce_adam": 3, "square_adam": 3, "bpr_adam": 3}          # every other case: 2
B_POINT, B_PAIR = 60, 40

_SHADOWED = ("util", "util.tool", "util.learner", "util.data_iterator", "data", "evaluator", "model",
             "model.AbstractRecommender", "model.sequential_recommender")


def load_transrec():
    """the reference module model/sequential_recommender/TransRec.py, executed under the shim (make_golden_fpmc.load_fpmc
    with util.data_iterator added: TransRec.py imports DataIterator from there)"""
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
        util.data_iterator = rm._load_file("util.data_iterator", os.path.join(rm.REF, "util", "data_iterator.py"))
        data = types.ModuleType("data")
        data.TimeOrderPointwiseSampler = data.TimeOrderPairwiseSampler = rm.ReplaySampler
        sys.modules["data"] = data
        ev = types.ModuleType("evaluator")
        ev.ProxyEvaluator = rm.RecordingEvaluator
        sys.modules["evaluator"] = ev
        model_pkg = types.ModuleType("model")
        model_pkg.__path__ = []
        sys.modules["model"] = model_pkg
        rm._load_file("model.AbstractRecommender", os.path.join(rm.REF, "model", "AbstractRecommender.py"))
        mod = rm._load_file("model.sequential_recommender.TransRec",
                            os.path.join(rm.REF, "model", "sequential_recommender", "TransRec.py"))
        sys.modules.pop("model.sequential_recommender.TransRec", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


def attach_ops():
    """ops of TransRec.py the shim lacks, by their published definitions, each checked here on a small value:
    tf.tile (the input repeated multiples[k] times along axis k), tf.norm(ord='euclidean', axis) (sqrt of the sum of
    squares over the axis) and a tf.stack that takes Python ints beside tensors — `tf.stack([batch_size, 1])` hands the
    shim's torch.stack an int"""
    import torch

    def tile(input, multiples, name=None):                  # noqa: A002
        return tf_shim.Tensor(lambda a, m: a.repeat(*[int(x) for x in m]), [input, multiples])

    def norm(tensor, ord="euclidean", axis=None, keepdims=None, name=None, keep_dims=None):   # noqa: A002
        assert ord in ("euclidean", 2), ord
        kd = True if (keepdims or keep_dims) else False
        ax = tf_shim._axes(axis)
        return tf_shim.Tensor(lambda a: torch.sqrt(torch.sum(a * a) if ax is None else
                                                   torch.sum(a * a, dim=ax, keepdim=kd)), [tensor])

    def stack(values, axis=0, name=None):
        return tf_shim.Tensor(lambda *xs: torch.stack([torch.as_tensor(x) for x in xs], dim=axis), list(values))

    tf_shim.tile, tf_shim.norm, tf_shim.stack = tile, norm, stack
    run = lambda t: tf_shim._evaluate([t], {})[0]
    x = torch.tensor([[1.0, 2.0]], dtype=torch.float64)
    n = tf_shim.shape(tf_shim.constant(np.zeros((3, 5))))[0]
    m = run(stack([n, 1]))
    assert m.tolist() == [3, 1], m
    assert run(tile(x, stack([n, 1]))).tolist() == [[1.0, 2.0]] * 3
    assert run(tile(x, [2, 2])).tolist() == [[1.0, 2.0, 1.0, 2.0]] * 2
    assert run(stack([x, x], axis=1)).shape == (1, 2, 2)                   # tensors as before
    y = torch.tensor([[[3.0, 4.0], [0.0, 0.0]], [[1.0, 0.0], [5.0, 12.0]]], dtype=torch.float64)
    assert run(norm(y, ord="euclidean", axis=-1)).tolist() == [[5.0, 0.0], [1.0, 13.0]]
    for name in ("multiply", "reduce_sum", "placeholder", "square", "expand_dims", "shape"):
        assert hasattr(tf_shim, name), name
    return True


def build(dataset, hyper, width):
    """ref_models.build for the sequential class"""
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    mod = load_transrec()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "TransRec"
    conf.update(hyper)
    sess = tf_shim.Session(seed=0)
    model = mod.TransRec(sess, dataset, conf)
    assert {u: list(s) for u, s in model.train_dict.items()} == dataset.seqs      # csr_to_user_dict_bytime
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess


# ------------------------------------------------------------------ inputs
def make_batches(seqs, n_items, steps, pairwise, seed):
    """[(users, recent, items, third)] per step: windows (seq[k], seq[k+1]) of the users' sequences, negatives and
    label-0 items outside the user's sequence, and one instance whose target is its own recent item; every batch holds
    the duplicate patterns of transrec_restatement.edge_patterns (checked)"""
    rs = np.random.RandomState(seed)
    windows = [(u, s[k], s[k + 1]) for u, s in seqs.items() for k in range(len(s) - 1)]
    long = [u for u, s in seqs.items() if len(s) >= 3]
    B = B_PAIR if pairwise else B_POINT

    def neg(u):
        while True:
            j = int(rs.randint(n_items))
            if j not in seqs[u]:
                return j

    out = []
    for _ in range(steps):
        u0 = long[rs.randint(len(long))]
        s0 = seqs[u0]
        # a user three times; s0[1] is a target, then a recent, then its own target
        pos = [(u0, s0[0], s0[1]), (u0, s0[1], s0[2]), (u0, s0[1], s0[1])]
        n_pos = B if pairwise else B // 2
        for k in rs.choice(len(windows), n_pos - len(pos), replace=False):
            pos.append(windows[k])
        if pairwise:
            negs = [neg(u) for u, _, _ in pos]
            for k in range(3, len(pos)):                          # s0[1] is some other user's negative as well
                if s0[1] not in seqs[pos[k][0]]:
                    negs[k] = s0[1]
                    break
            users, recent, items = ([p[c] for p in pos] for c in range(3))
            third = np.asarray(negs, np.int32)
        else:
            inst = [(u, l, i, 1.0) for u, l, i in pos] + [(u, l, neg(u), 0.0) for u, l, _ in pos]
            inst = [inst[k] for k in rs.permutation(len(inst))]
            users, recent, items = ([p[c] for p in inst] for c in range(3))
            third = np.asarray([p[3] for p in inst], np.float32)
        assert len(users) == B
        pat = P.edge_patterns(users, recent, items, third, pairwise)
        assert all(pat.values()), pat
        out.append(tuple(np.asarray(x, np.int32) for x in (users, recent, items)) + (third,))
    return out


# ------------------------------------------------------------------ the runs
def _variables(model):
    return (model.user_embeddings, model.item_embeddings, model.item_biases, model.global_embedding)


def run_case(ds, init, hyper, batches, predict_users=None, cand=None):
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, hyper, width)
        for var, t in zip(_variables(model), init):
            var.load(t)
        tabs, losses = [], []
        for users, recent, items, third in batches:
            feed = {model.user_input: users, model.item_input: items, model.item_input_recent: recent}
            feed[model.item_input_neg if hyper["is_pairwise"] else model.labels] = third
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=feed)
            losses.append(float(loss))
            tabs.append(tuple(v.numpy() for v in _variables(model)))
        out[tag] = (tabs, np.asarray(losses, np.float64))
        if predict_users is not None:
            out[tag + "_predict"] = _np(model.predict(list(predict_users), None), width)
            out[tag + "_predict_cand"] = _np(model.predict(list(predict_users), [list(c) for c in cand]), width)
    return out


def pack(case, res, init, batches):
    """rows that moved, per table, and their DIFFERENCE from the initial table in float64 (make_golden_fpmc.pack); T is
    stored whole"""
    init64 = [t.astype(np.float64) for t in init]
    out = {case + "_" + name: np.stack([b[c] for b in batches])
           for c, name in enumerate(("users", "recent", "items", "third"))}
    for j, name in enumerate(P.TABLES):
        if name == "T":
            rows = np.arange(1, dtype=np.int32)
        else:
            moved = np.zeros(len(init[j]), bool)
            for tag, _ in WIDTHS:
                for tabs in res[tag][0]:
                    diff = tabs[j].astype(np.float64) != init64[j]
                    moved |= diff.reshape(len(diff), -1).any(axis=1)
            rows = np.flatnonzero(moved).astype(np.int32)
            out["%s_rows_%s" % (case, name)] = rows
        for tag, width in WIDTHS:
            delta = np.stack([t[j].astype(np.float64)[rows] - init64[j][rows] for t in res[tag][0]])
            back = (init64[j][rows][None] + delta).astype(np.float32 if width == "float32" else np.float64)
            want = np.stack([t[j][rows] for t in res[tag][0]])
            assert np.array_equal(back, want) if width == "float32" else np.abs(back - want).max(initial=0) < 1e-15
            out["%s_%s_%s" % (case, tag, name)] = delta
    for tag, _ in WIDTHS:
        out["%s_%s_loss" % (case, tag)] = res[tag][1]
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_ops()
    R = toy_matrix()
    U, I = R.shape
    seqs = time_orders(R)
    ds = TimedDataset(R, seqs)
    d = HYPER["embedding_size"]
    rs = np.random.RandomState(4217)
    init = [(0.1 * rs.randn(*shape)).astype(np.float32) for shape in ((U, d), (I, d), (I,), (1, d))]
    not_max = [u for u, s in seqs.items() if len(s) >= 2 and s[-1] != max(s)]
    is_max = [u for u, s in seqs.items() if len(s) >= 2 and s[-1] == max(s)]
    single = [u for u, s in seqs.items() if len(s) == 1]
    predict_users = np.asarray(not_max[:3] + is_max[:1] + single[:1], np.int32)
    cand = np.asarray([[3, 0, I - 1], [7, 7, 1], [0, 1, 2], [I - 1, I - 2, 5], [9, 8, 0]], np.int32)
    ptr = np.zeros(U + 1, np.int64)
    for u, s in seqs.items():
        ptr[u + 1] = len(s)
    ptr = np.cumsum(ptr)
    out = dict(indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32), shape=np.asarray(R.shape, np.int64),
               seq_ptr=ptr, seq=np.asarray([i for u in sorted(seqs) for i in seqs[u]], np.int32),
               P_0=init[0], Q_0=init[1], b_0=init[2], T_0=init[3], predict_users=predict_users, predict_cand=cand,
               learning_rate=np.float64(HYPER["learning_rate"]), cases=np.asarray(sorted(P.CASES)))
    gaps = {}
    for k, case in enumerate(sorted(P.CASES)):
        loss, learner, pairwise, reg = P.CASES[case]
        hyper = dict(HYPER, loss_function=loss, learner=learner, is_pairwise=pairwise, reg_mf=reg)
        batches = make_batches(seqs, I, STEPS.get(case, 2), pairwise, seed=500 + k)
        last = case == P.PREDICT_CASE
        res = run_case(ds, init, hyper, batches, predict_users if last else None, cand if last else None)
        out.update(pack(case, res, init, batches))
        out[case + "_reg_mf"] = np.float64(reg)
        if last:
            for tag, _ in WIDTHS:
                out["predict_" + tag] = res[tag + "_predict"]
                out["predict_cand_" + tag] = res[tag + "_predict_cand"]
        gaps[case] = max(np.abs(out["%s_f32_%s" % (case, t)] - out["%s_f64_%s" % (case, t)]).max() for t in P.TABLES)
    path = os.path.join(HERE, "tfgraph_transrec.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); fp32 vs fp64 table gaps %s; predict gap %.3g" % (
        path, os.path.getsize(path), {k: "%.3g" % v for k, v in gaps.items()},
        np.abs(out["predict_f32"] - out["predict_f64"]).max()))


if __name__ == "__main__":
    main()
