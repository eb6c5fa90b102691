"""Golden APR trace produced by the REFERENCE's own APR class (model/general_recommender/APR.py).

The class is loaded whole and unchanged with oracle/ref_models.load (its `_load_file`) and runs under oracle/tf_shim.py
on toy_matrix().  The class builds an adversarial graph that its own train_model() never runs (APR.py:122, 132-150), so
for the adversarial cases the maker drives the class's own nodes itself, the way the paper runs them:

    sess.run([model.update_P, model.update_Q], feed)                  # Delta from this batch at the current tables
    sess.run((model.loss, model.opt_loss, opt), feed)                 # opt = learner.optimizer(.., model.opt_loss, lr)

The shim lacks four things APR.py uses, attached here and each first put on a hand-computed value (attach_ops):
Variable.assign, tf.gradients (a node that differentiates under the feeds of the running session — FeedSession holds
them), tf.stop_gradient and tf.truncated_normal (through Session.draw, so the draws are recorded).

    python tests/golden/make_golden_apr.py              # needs the reference tree

Writes tests/golden/tfgraph_apr.npz:
  indptr / indices / shape       the train pattern: toy_matrix() (157 x 131)
  cases, learning_rate
  <case>_P_0 / <case>_Q_0        the case's initial tables (0.1 randn, float32); <case>_users/_pos/_neg [steps, 48]
  <case>_rows_{P,Q}              the rows of that table that differ from the initial value at any step, in either width
                                 (<case>_every_row_moved: the cases with the dense regulariser hold whole tables; an
                                 Adam sweep leaves a row with zero gradient and zero moments where it is)
  <case>_{f32,f64}_{P,Q}         [steps, len(rows), d]: those rows after each step MINUS their initial value, float64
  <case>_{f32,f64}_loss / _opt_loss   [steps]: the fetched (pre-update) values
  <case>_drows_{P,Q}_<s>, <case>_{f32,f64}_delta_{P,Q}_<s>   adversarial cases: the batch's rows of step s and Delta there
                                 (every other row of delta_P / delta_Q is zero: checked)
  random_adam_draw_{P,Q}_<s>     the truncated-normal draws of the batch's rows (float32, the same in both widths)
  epoch_*                        one whole train_model() epoch of the class as shipped, batch_size 64: the fed batches
                                 (flat, epoch_sizes), per-step losses, the logged figure, the end tables as differences
  predict_users, predict_cand, predict_{f32,f64}, predict_cand_{f32,f64}   predict() after that epoch, both modes
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_models as rm          # noqa: E402
from oracle import tf_shim                    # noqa: E402
from make_golden_tfgraph import WIDTHS, _np, _reset_recorders, toy_matrix   # noqa: E402
import apr_restatement as A                   # noqa: E402

HYPER = dict(epochs=1, batch_size=64, embedding_size=16, reg=0.0, reg_adv=1.0, learning_rate=A.LR, learner="adam",
             adv_epoch=0, adv="grad", eps=0.5, adver=1, init_method="tnormal", stddev=0.01, verbose=1)
EPOCH_HYPER = dict(HYPER, reg=0.05)


class FeedSession(tf_shim.Session):
    """the shim's Session that holds the feeds of the running call (the `gradients` node differentiates under them),
    logs them, and draws `truncated_normal` inputs like the other random inputs: queued or fresh, and recorded"""

    def __init__(self, **k):
        tf_shim.Session.__init__(self, **k)
        self.feeds, self.fed, self.fetched = {}, [], []

    def run(self, fetches, feed_dict=None):
        self.feeds = dict(feed_dict or {})
        if feed_dict:
            self.fed.append(feed_dict)
        out = tf_shim.Session.run(self, fetches, feed_dict)
        self.fetched.append(out)
        return out

    def draw(self, kind, shape, **p):
        if kind != "truncated_normal" or self._queue:
            return tf_shim.Session.draw(self, kind, shape, **p)
        a = self.rng.randn(*shape)
        while (np.abs(a) > 2).any():                           # values beyond two standard deviations are redrawn
            bad = np.abs(a) > 2
            a[bad] = self.rng.randn(int(bad.sum()))
        a = (p["mean"] + p["stddev"] * a).astype(np.float32)
        self.draw_log.append((kind, a))
        return a


def attach_ops():
    import torch
    T = tf_shim.Tensor

    def assign_method(self, value, use_locking=None, name=None, read_value=True):
        return tf_shim.assign(self, value)

    def stop_gradient(input, name=None):                   # noqa: A002
        return T(lambda a: a.detach(), [input])

    def gradients(ys, xs, **_):
        """d ys / d x per variable x, DENSE: the backward of a lookup sums the rows of a repeated id into the variable's
        row (what tf.stop_gradient makes of the IndexedSlices, APR.py:112-114)"""
        xs = list(xs)
        assert all(isinstance(x, tf_shim.Variable) for x in xs)

        def node(x):
            def f():
                sess = tf_shim._RUN["session"]
                feeds = {id(k): v for k, v in sess.feeds.items()}
                with torch.enable_grad():
                    leaves = {id(v): v.value.detach().clone().requires_grad_(True) for v in xs}
                    y = tf_shim._evaluate([ys], feeds, leaves)[0]
                    g = torch.autograd.grad(y, leaves[id(x)])[0]
                return g.detach()
            return T(f, [])
        return [node(x) for x in xs]

    def truncated_normal(shape, mean=0.0, stddev=1.0, dtype=None, seed=None, name=None):
        shp = tuple(int(s) for s in shape)
        return T(lambda: tf_shim._to_torch(tf_shim._RUN["session"].draw("truncated_normal", shp, mean=mean,
                                                                          stddev=stddev)), [])

    tf_shim.Variable.assign = assign_method
    tf_shim.stop_gradient, tf_shim.gradients, tf_shim.truncated_normal = stop_gradient, gradients, truncated_normal
    # ---- each on a hand-computed value
    tf = tf_shim
    tf.set_float("float64")
    tf.reset_default_graph()
    sess = FeedSession(seed=3)
    v = tf.Variable(np.asarray([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]), name="v")
    ids = tf.placeholder(tf.int32, shape=[None])
    w = tf.constant(np.asarray([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]]))
    loss = tf.reduce_sum(tf.nn.embedding_lookup(v, ids) * w)
    (gv,) = tf.gradients(loss, [v])
    got = sess.run(tf.stop_gradient(gv), {ids: [2, 0, 2]})
    assert got.tolist() == [[2.0, 2.0], [0.0, 0.0], [4.0, 4.0]], got       # id 2 twice: 1 + 3 in ONE dense row
    got = sess.run(gv, {ids: [1, 1, 1]})                                   # the node follows the feeds of each run
    assert got.tolist() == [[0.0, 0.0], [6.0, 6.0], [0.0, 0.0]], got
    target = tf.Variable(tf.zeros(shape=[3, 2]), trainable=False)
    assert sess.run(target.assign(tf.nn.l2_normalize(tf.stop_gradient(gv), 1) * 0.5), {ids: [2, 0, 2]}) is None
    r = 0.5 / np.sqrt(2.0)
    assert np.allclose(target.numpy(), [[r, r], [0.0, 0.0], [r, r]], rtol=0, atol=1e-16), target.numpy()
    x = tf.Variable(np.asarray([2.0]))
    y = tf.reduce_sum(x * tf.stop_gradient(x * x))                         # d/dx = x^2 with the factor held constant
    sess.run(tf.train.GradientDescentOptimizer(1.0).minimize(y))
    assert x.numpy().tolist() == [2.0 - 4.0], x.numpy()
    tn = sess.run(tf.truncated_normal(shape=[400, 5], mean=0.0, stddev=0.01))
    assert tn.shape == (400, 5) and np.abs(tn).max() <= 0.02 + 1e-9 and 0.006 < tn.std() < 0.01
    assert sess.draw_log[-1][0] == "truncated_normal" and np.array_equal(sess.draw_log[-1][1].astype(np.float64), tn)
    sess.inject([np.full((2, 2), 0.015, np.float32)])
    assert sess.run(tf.truncated_normal(shape=[2, 2], stddev=0.01)).tolist() == [[np.float32(0.015)] * 2] * 2
    tf.reset_default_graph()
    return True


def build(dataset, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    mod = rm.load("APR")
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "APR"
    conf.update(hyper)
    sess = FeedSession(seed=11)
    model = mod.APR(sess, dataset, conf)
    saved = tf_shim.install()                                  # build_graph and the maker's optimizer call `tf.*`
    try:
        model.build_graph()
    finally:
        tf_shim.uninstall(saved)
    sess.run(tf_shim.global_variables_initializer())
    return model, sess, mod


# ------------------------------------------------------------------ inputs
def make_batches(R, steps, seed, B=A.BATCH):
    """[(users, pos, neg)] per step: train pairs with uniform negatives outside the user's row, and in every batch a
    user three times, an item that is positive in one triplet and negative in another, a (user, positive) pair twice"""
    rs = np.random.RandomState(seed)
    U, I = R.shape
    rows = {u: R.indices[R.indptr[u]:R.indptr[u + 1]].tolist() for u in range(U)}
    pairs = [(u, i) for u, its in rows.items() for i in its]
    rich = [u for u, its in rows.items() if len(its) >= 3]

    def neg(u):
        while True:
            j = int(rs.randint(I))
            if j not in rows[u]:
                return j

    out = []
    for _ in range(steps):
        u0 = rich[rs.randint(len(rich))]
        trip = [(u0, rows[u0][0]), (u0, rows[u0][1]), (u0, rows[u0][1])]          # a user three times, a pair twice
        trip += [pairs[k] for k in rs.choice(len(pairs), B - len(trip), replace=False)]
        negs = [neg(u) for u, _ in trip]
        target = rows[u0][0]
        for k in range(3, B):                                  # rows[u0][0] is some other user's negative as well
            if target not in rows[trip[k][0]]:
                negs[k] = target
                break
        users, pos = (np.asarray([t[c] for t in trip], np.int32) for c in range(2))
        negs = np.asarray(negs, np.int32)
        pat = A.edge_patterns(users, pos, negs)
        assert all(pat.values()), pat
        out.append((users, pos, negs))
    return out


def epoch_batches(R, seed, B=64):
    rs = np.random.RandomState(seed)
    U, I = R.shape
    rows = {u: set(R.indices[R.indptr[u]:R.indptr[u + 1]].tolist()) for u in range(U)}
    coo = R.tocoo()
    order = rs.permutation(coo.nnz)
    users, pos = coo.row[order].astype(np.int32), coo.col[order].astype(np.int32)
    neg = np.empty_like(pos)
    for k, u in enumerate(users):
        while True:
            j = int(rs.randint(I))
            if j not in rows[int(u)]:
                neg[k] = j
                break
    return [(users[a:a + B], pos[a:a + B], neg[a:a + B]) for a in range(0, len(users), B)]


# ------------------------------------------------------------------ the runs
def run_case(ds, case, init, batches):
    adv, learner_name, d, reg, reg_adv, eps = A.CASES[case]
    hyper = dict(HYPER, embedding_size=d, learner=learner_name, reg=reg, reg_adv=reg_adv, eps=eps,
                 adv="random" if adv == "random" else "grad", adver=0 if adv is None else 1)
    out = {}
    draws = None
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess, mod = build(ds, hyper, width)
        model.embedding_P.load(init[0])
        model.embedding_Q.load(init[1])
        assert not model.delta_P.numpy().any() and not model.delta_Q.numpy().any()
        if adv == "shipped":
            opt = model.optimizer
        else:
            saved = tf_shim.install()
            try:
                opt = mod.learner.optimizer(model.learner, model.opt_loss, model.learning_rate)
            finally:
                tf_shim.uninstall(saved)
        if adv == "random" and draws is not None:
            sess.inject([a for _, a in draws])                   # the float64 twin runs on the float32 run's draws
        tabs, losses, opts, deltas = [], [], [], []
        for users, pos, neg in batches:
            feed = {model.user_input: users, model.item_input_pos: pos, model.item_input_neg: neg}
            if adv in ("grad", "random"):
                sess.run([model.update_P, model.update_Q], feed)
                rows_p, rows_q = A.batch_rows(init[0], init[1], users, pos, neg)
                dP, dQ = model.delta_P.numpy(), model.delta_Q.numpy()
                if adv == "grad":                              # a row outside the batch has Delta = 0
                    for full, rows in ((dP, rows_p), (dQ, rows_q)):
                        rest = np.setdiff1d(np.arange(len(full)), rows)
                        assert not full[rest].any() and full[rows].any(axis=1).all()
                deltas.append((rows_p, dP[rows_p], rows_q, dQ[rows_q]))
            loss, opt_loss, _ = sess.run((model.loss, model.opt_loss, opt), feed)
            losses.append(float(loss))
            opts.append(float(opt_loss))
            tabs.append((model.embedding_P.numpy(), model.embedding_Q.numpy()))
        if adv == "random":
            if draws is None:
                draws = list(sess.draw_log)
            assert len(sess.draw_log) == 2 * len(batches) and all(k == "truncated_normal" for k, _ in sess.draw_log)
        if adv == "shipped":                                   # the graph's Delta variables were never assigned
            assert not model.delta_P.numpy().any() and not model.delta_Q.numpy().any()
        out[tag] = (tabs, np.asarray(losses), np.asarray(opts), deltas)
    out["draws"] = draws
    return out


def pack_tables(prefix, res_tabs, init):
    """rows that moved in either width and their difference from the initial table in float64
    (make_golden_transrec.pack)"""
    init64 = [t.astype(np.float64) for t in init]
    out = {}
    for j, name in enumerate(("P", "Q")):
        moved = np.zeros(len(init[j]), bool)
        for tag, _ in WIDTHS:
            for tabs in res_tabs[tag]:
                moved |= (tabs[j].astype(np.float64) != init64[j]).any(axis=1)
        rows = np.flatnonzero(moved).astype(np.int32)
        out["%s_rows_%s" % (prefix, name)] = rows
        for tag, width in WIDTHS:
            delta = np.stack([t[j].astype(np.float64)[rows] - init64[j][rows] for t in res_tabs[tag]])
            back = (init64[j][rows][None] + delta).astype(np.float32 if width == "float32" else np.float64)
            want = np.stack([t[j][rows] for t in res_tabs[tag]])
            assert np.array_equal(back, want) if width == "float32" else np.abs(back - want).max(initial=0) < 1e-15
            out["%s_%s_%s" % (prefix, tag, name)] = delta
    return out


def run_epoch(ds, init, batches, predict_users, cand):
    """the class as shipped: train_model() itself, one epoch over the replayed batches"""
    out = {"epoch_users": np.concatenate([b[0] for b in batches]), "epoch_pos": np.concatenate([b[1] for b in batches]),
           "epoch_neg": np.concatenate([b[2] for b in batches]),
           "epoch_sizes": np.asarray([len(b[0]) for b in batches], np.int32)}
    tabs = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        rm.ReplaySampler.batches = batches
        rm.RecordingEvaluator.users = list(predict_users)
        model, sess, _ = build(ds, EPOCH_HYPER, width)
        model.embedding_P.load(init[0])
        model.embedding_Q.load(init[1])
        model.train_model()
        assert len(sess.fed) == len(batches)
        for feed, b in zip(sess.fed, batches):                   # what the class fed is what the file holds
            assert np.array_equal(feed[model.user_input], b[0]) and np.array_equal(feed[model.item_input_neg], b[2])
        losses = np.asarray([float(f[0]) for f in sess.fetched if isinstance(f, list) and len(f) == 2 and f[1] is None])
        assert len(losses) == len(batches)
        line = [ln for ln in rm.MemoryLogger.lines if ln.startswith("[iter 1 :")]
        assert len(line) == 1
        out["epoch_%s_losses" % tag] = losses
        out["epoch_%s_logged" % tag] = np.float64(re.match(r"\[iter 1 : loss : ([-0-9.e]+),", line[0]).group(1))
        tabs[tag] = [(model.embedding_P.numpy(), model.embedding_Q.numpy())]
        assert not model.delta_P.numpy().any()
        out["predict_" + tag] = _np(model.predict(list(predict_users), None), width)
        out["predict_cand_" + tag] = _np(model.predict(list(predict_users), [list(c) for c in cand]), width)
        assert np.array_equal(rm.RecordingEvaluator.ratings[-1], out["predict_" + tag])
    out.update(pack_tables("epoch", tabs, init))
    rm.ReplaySampler.batches = []
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_ops()
    R = toy_matrix()
    U, I = R.shape
    ds = rm.Dataset(R)
    out = dict(indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32), shape=np.asarray(R.shape, np.int64),
               learning_rate=np.float64(A.LR), cases=np.asarray(sorted(A.CASES)))
    gaps = {}
    for k, case in enumerate(sorted(A.CASES)):
        d = A.CASES[case][2]
        rs = np.random.RandomState(8100 + k)
        init = [(0.1 * rs.randn(U, d)).astype(np.float32), (0.1 * rs.randn(I, d)).astype(np.float32)]
        batches = make_batches(R, A.STEPS, seed=900 + k)
        res = run_case(ds, case, init, batches)
        out[case + "_P_0"], out[case + "_Q_0"] = init
        for c, name in enumerate(("users", "pos", "neg")):
            out["%s_%s" % (case, name)] = np.stack([b[c] for b in batches])
        out.update(pack_tables(case, {tag: res[tag][0] for tag, _ in WIDTHS}, init))
        # Adam sweeps every row, but a row whose gradient and moments are still zero stays where it is: only the dense
        # regulariser (reg != 0 outside the shipped loop) moves every row, and that case holds whole tables
        whole = len(out[case + "_rows_P"]) == U and len(out[case + "_rows_Q"]) == I
        assert whole == (A.CASES[case][3] != 0 and A.CASES[case][0] != "shipped")
        out[case + "_every_row_moved"] = np.bool_(whole)
        for tag, _ in WIDTHS:
            out["%s_%s_loss" % (case, tag)], out["%s_%s_opt_loss" % (case, tag)] = res[tag][1], res[tag][2]
            for s, dl in enumerate(res[tag][3]):
                out["%s_drows_P_%d" % (case, s)], out["%s_drows_Q_%d" % (case, s)] = \
                    dl[0].astype(np.int32), dl[2].astype(np.int32)
                out["%s_%s_delta_P_%d" % (case, tag, s)] = dl[1].astype(np.float64)
                out["%s_%s_delta_Q_%d" % (case, tag, s)] = dl[3].astype(np.float64)
        if res["draws"] is not None:
            for s in range(A.STEPS):
                out["%s_draw_P_%d" % (case, s)] = res["draws"][2 * s][1][out["%s_drows_P_%d" % (case, s)]]
                out["%s_draw_Q_%d" % (case, s)] = res["draws"][2 * s + 1][1][out["%s_drows_Q_%d" % (case, s)]]
        gaps[case] = max(np.abs(out["%s_f32_%s" % (case, t)] - out["%s_f64_%s" % (case, t)]).max() for t in "PQ")
    rs = np.random.RandomState(8200)
    d = EPOCH_HYPER["embedding_size"]
    init = [(0.1 * rs.randn(U, d)).astype(np.float32), (0.1 * rs.randn(I, d)).astype(np.float32)]
    predict_users = np.asarray(sorted(rs.choice(U, 27, replace=False)), np.int32)
    cand = rs.randint(0, I, (27, 3)).astype(np.int32)
    out.update(epoch_P_0=init[0], epoch_Q_0=init[1], predict_users=predict_users, predict_cand=cand)
    out.update(run_epoch(ds, init, epoch_batches(R, seed=77), predict_users, cand))
    path = os.path.join(HERE, "tfgraph_apr.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); fp32 vs fp64 table gaps %s; predict gap %.3g" % (
        path, os.path.getsize(path), {k: "%.3g" % v for k, v in gaps.items()},
        np.abs(out["predict_f32"] - out["predict_f64"]).max()))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
