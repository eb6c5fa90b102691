"""Golden SBPR trace produced by the REFERENCE's own SBPR class (model/social_recommender/SBPR.py).

The class and model/AbstractRecommender.py (SocialAbstractRecommender reads the trust file with pandas) are loaded whole
and unchanged with oracle/ref_models._load_file and run under oracle/tf_shim.py, as make_golden_transrec.py does for
TransRec: the same stand-ins (`util` re-exporting the reference's tool / learner functions, `evaluator`, `model`) plus
the reference's own util/data_iterator.py.  tf.gather, which the shim lacks, is attached at run time by its published
definition (array_ops.gather on axis 0 = the shim's embedding_lookup), as make_golden_irgan.py does; nothing under
oracle/ changes.  The maker drives `sess.run((model.loss, model.optimizer), feed_dict)` itself; train_model() is not
called.  _get_SocialItemsSet(), _get_pairwise_all_data() and predict() are the reference's.

    python tests/golden/make_golden_sbpr.py              # needs the reference tree, pandas and scipy

Writes tests/golden/tfgraph_sbpr.npz:
  indptr / indices / shape     the train pattern: toy_matrix() (157 x 131)
  trust_lines [n, 2]           the trust file as written (sbpr_restatement.trust_graph: users who trust nobody, users
                               who trust themselves, duplicated lines, no edge to a user without train items)
  trust_indptr / trust_indices the reference's social_matrix (deduplicated)
  social_ptr / social_items    the reference's userSocialItemsSetList, items ascending per user
  epoch_users/_items/_social/_neg/_suk   one _get_pairwise_all_data() under np.random.seed(EPOCH_SEED)
  P_0 / Q_0 / b_0              the initial tables (0.1 randn); hyper-parameters as scalars
  <case>_users/_items/_social/_neg/_suk  the batches [steps, B]
  <case>_rows_{P,Q,b}          the rows of that table that differ from its initial value at any step, in either width —
                               every other row equals its initial value after every step
  <case>_{f32,f64}_{P,Q,b}     [steps, len(rows), ...]: those rows after each step MINUS their initial value, in
                               float64; <case>_{f32,f64}_loss [steps]: the fetched (pre-update) loss
  predict_users, predict_{f32,f64}, predict_cand, predict_cand_{f32,f64}
                               predict() rows after the last step of the case `bpr_adam`, full and candidate mode
"""
import os
import sys
import tempfile
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
import sbpr_restatement as P                  # noqa: E402

HYPER = dict(learning_rate=0.01, embedding_size=16, learner="adam", loss_function="bpr", num_epochs=1, reg_mf=P.REG,
             batch_size=48, init_method="normal", stddev=0.01, verbose=1, topk=20)
BATCH = 48
EPOCH_SEED = 77
SEPARATOR = ","

_SHADOWED = ("util", "util.tool", "util.learner", "util.data_iterator", "evaluator", "model",
             "model.AbstractRecommender", "model.social_recommender")


def load_sbpr():
    """the reference module model/social_recommender/SBPR.py, executed under the shim"""
    saved_tf = tf_shim.install()
    saved = {k: sys.modules.get(k) for k in _SHADOWED}
    try:
        tool = rm._load_file("util.tool", os.path.join(rm.REF, "util", "tool.py"))
        learner = rm._load_file("util.learner", os.path.join(rm.REF, "util", "learner.py"))
        util = types.ModuleType("util")
        util.__path__ = []
        util.tool, util.learner = tool, learner
        for fn in ("timer", "l2_loss", "csr_to_user_dict", "randint_choice"):
            setattr(util, fn, getattr(tool, fn))
        util.Logger = rm.MemoryLogger
        sys.modules["util"] = util
        util.data_iterator = rm._load_file("util.data_iterator", os.path.join(rm.REF, "util", "data_iterator.py"))
        ev = types.ModuleType("evaluator")
        ev.ProxyEvaluator = rm.RecordingEvaluator
        sys.modules["evaluator"] = ev
        model_pkg = types.ModuleType("model")
        model_pkg.__path__ = []
        sys.modules["model"] = model_pkg
        rm._load_file("model.AbstractRecommender", os.path.join(rm.REF, "model", "AbstractRecommender.py"))
        mod = rm._load_file("model.social_recommender.SBPR",
                            os.path.join(rm.REF, "model", "social_recommender", "SBPR.py"))
        sys.modules.pop("model.social_recommender.SBPR", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


def attach_ops():
    """tf.gather by its published definition, checked on a small value; tf.divide is the shim's"""
    if not hasattr(tf_shim, "gather"):
        def gather(params, indices, name=None, **_):
            return tf_shim.nn.embedding_lookup(params, indices)
        tf_shim.gather = gather
    tf = tf_shim
    tf.set_float("float64")
    tf.reset_default_graph()
    sess = tf.Session(seed=0)
    v = tf.Variable(np.asarray([1.0, 2.0, 4.0]))
    ids = tf.placeholder(tf.int32)
    assert sess.run(tf.gather(v, ids), {ids: [2, 0, 2]}).tolist() == [4.0, 1.0, 4.0]
    assert sess.run(tf.divide(tf.gather(v, ids), tf.constant(np.asarray([2.0, 4.0]))), {ids: [2, 0]}).tolist() == \
        [2.0, 0.25]
    tf.reset_default_graph()
    return True


class SocialDataset(rm.Dataset):
    """rm.Dataset with the `userids` map of data/dataset.py: raw id -> row; here the identity on integers"""

    def __init__(self, train):
        rm.Dataset.__init__(self, train)
        self.userids = {u: u for u in range(self.num_users)}


def build(dataset, hyper, width, social_file):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    mod = load_sbpr()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "SBPR"
    conf["social_file"] = social_file
    conf["data.convert.separator"] = SEPARATOR
    conf.update(hyper)
    sess = tf_shim.Session(seed=0)
    model = mod.SBPR(sess, dataset, conf)
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess


def _variables(model):
    return (model.user_embeddings, model.item_embeddings, model.bias)


# ------------------------------------------------------------------ inputs
def make_batches(epoch, steps, seed):
    """[(users, items, social, neg, suk)] per step: BATCH instances of the recorded epoch, drawn without replacement"""
    rs = np.random.RandomState(seed)
    n = len(epoch[0])
    out = []
    for _ in range(steps):
        pick = rs.choice(n, BATCH, replace=False)
        out.append(tuple(np.asarray(f)[pick] for f in epoch))
    return out


def dup_batch(epoch):
    """one batch in which one item occurs as i, as k and as j of different slots and a user occurs several times:
    the recorded epoch's instances of the user with the most of them, then three slots of other users re-pointed at the
    item x = that user's first positive (the graph takes any ids)"""
    users, items, social, neg, suk = (np.asarray(f).copy() for f in epoch)
    u0 = np.bincount(users).argmax()
    own = np.flatnonzero(users == u0)[:6]
    rest = np.flatnonzero(users != u0)[:BATCH - len(own)]
    pick = np.concatenate([own, rest])
    b = [f[pick] for f in (users, items, social, neg, suk)]
    x = b[1][0]
    n = len(own)
    b[2][n] = x                                               # x is a social item there
    b[3][n + 1] = x                                           # and a negative there
    b[1][n + 2] = x                                           # and another user's positive
    assert len(set(b[0].tolist())) < len(b[0]) and x in b[1] and x in b[2] and x in b[3]
    return [tuple(b)]


def run_case(ds, init, hyper, batches, social_file, predict_users=None, cand=None):
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, hyper, width, social_file)
        for var, t in zip(_variables(model), init):
            var.load(t)
        tabs, losses = [], []
        for users, items, social, neg, suk in batches:
            feed = {model.user_input: users, model.item_input_pos: items, model.item_input_social: social,
                    model.item_input_neg: neg, model.suk: suk}
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=feed)
            losses.append(float(loss))
            tabs.append(tuple(v.numpy() for v in _variables(model)))
        out[tag] = (tabs, np.asarray(losses, np.float64))
        if predict_users is not None:
            # evaluate() (SBPR.py:152) fetches the tables before the evaluator calls predict()
            model._cur_user_embeddings, model._cur_item_embeddings = sess.run([model.user_embeddings,
                                                                               model.item_embeddings])
            out[tag + "_predict"] = _np(model.predict(list(predict_users), None), width)
            out[tag + "_predict_cand"] = _np(model.predict(list(predict_users), [list(c) for c in cand]), width)
    return out


def pack(case, res, init, batches):
    """rows that moved, per table, and their DIFFERENCE from the initial table in float64 (make_golden_transrec.pack)"""
    init64 = [t.astype(np.float64) for t in init]
    out = {}
    for c, name in enumerate(("users", "items", "social", "neg")):
        out[case + "_" + name] = np.stack([b[c] for b in batches]).astype(np.int32)
    out[case + "_suk"] = np.stack([b[4] for b in batches]).astype(np.float32)
    for j, name in enumerate(P.TABLES):
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
    ds = SocialDataset(R)
    lines = P.trust_graph(R)
    # what the graph must hold for the reference to run and for the trace to cover the quirks
    deg_tr = np.diff(R.indptr)
    srcs = set(u for u, _ in lines)
    assert len(srcs) < U and any(u == f for u, f in lines) and len(set(lines)) < len(lines)
    assert all(deg_tr[f] > 0 for _, f in lines), "an edge to a user without train items: the reference raises KeyError"
    d = HYPER["embedding_size"]
    rs = np.random.RandomState(4219)
    init = [(0.1 * rs.randn(*shape)).astype(np.float32) for shape in ((U, d), (I, d), (I,))]
    with tempfile.TemporaryDirectory() as tmp:
        social_file = os.path.join(tmp, "toy.uu")
        with open(social_file, "w") as f:
            for u, v in lines:
                f.write("%d%s%d\n" % (u, SEPARATOR, v))
        _reset_recorders()
        model, _ = build(ds, HYPER, "float64", social_file)
        S = model.social_matrix.tocsr()
        S.sort_indices()
        sets = {u: sorted(int(k) for k in items) for u, items in model.userSocialItemsSetList.items()}
        n_train_users = int((deg_tr > 0).sum())
        free = min(I - deg_tr[u] - len(s) for u, s in sets.items())
        assert 0 < len(sets) < n_train_users and free >= 1
        np.random.seed(EPOCH_SEED)
        epoch = model._get_pairwise_all_data()
        assert len(epoch[0]) == sum(int(deg_tr[u]) for u in sets)
        social_ptr = np.zeros(U + 1, np.int64)
        for u, s in sets.items():
            social_ptr[u + 1] = len(s)
        predict_users = np.asarray(sorted(sets)[:3] + [u for u in range(U) if u not in sets][:2], np.int32)
        cand = np.asarray([[3, 0, I - 1], [7, 7, 1], [0, 1, 2], [I - 1, I - 2, 5], [9, 8, 0]], np.int32)
        out = dict(indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32),
                   shape=np.asarray(R.shape, np.int64), trust_lines=np.asarray(lines, np.int32),
                   trust_indptr=S.indptr.astype(np.int64), trust_indices=S.indices.astype(np.int32),
                   social_ptr=np.cumsum(social_ptr),
                   social_items=np.asarray([k for u in sorted(sets) for k in sets[u]], np.int32),
                   epoch_users=np.asarray(epoch[0], np.int32), epoch_items=np.asarray(epoch[1], np.int32),
                   epoch_social=np.asarray(epoch[2], np.int32), epoch_neg=np.asarray(epoch[3], np.int32),
                   epoch_suk=np.asarray(epoch[4], np.float32),
                   P_0=init[0], Q_0=init[1], b_0=init[2], predict_users=predict_users, predict_cand=cand,
                   learning_rate=np.float64(HYPER["learning_rate"]), reg_mf=np.float64(P.REG),
                   cases=np.asarray(sorted(P.CASES)))
        gaps = {}
        for k, case in enumerate(sorted(P.CASES)):
            loss, learner = P.CASES[case]
            hyper = dict(HYPER, loss_function=loss, learner=learner)
            batches = dup_batch(epoch) if case == "bpr_adam_dup" else \
                make_batches(epoch, P.STEPS.get(case, 2), seed=700 + k)
            last = case == P.PREDICT_CASE
            res = run_case(ds, init, hyper, batches, social_file, predict_users if last else None,
                           cand if last else None)
            out.update(pack(case, res, init, batches))
            if last:
                for tag, _ in WIDTHS:
                    out["predict_" + tag] = res[tag + "_predict"]
                    out["predict_cand_" + tag] = res[tag + "_predict_cand"]
            gaps[case] = max(np.abs(out["%s_f32_%s" % (case, t)] - out["%s_f64_%s" % (case, t)]).max()
                             for t in P.TABLES)
    path = os.path.join(HERE, "tfgraph_sbpr.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); %d of %d train users eligible, %d instances, %d social entries, suk up to %d, at least "
          "%d free items; fp32 vs fp64 table gaps %s" % (
              path, os.path.getsize(path), len(sets), n_train_users, len(epoch[0]), len(out["social_items"]),
              int(max(epoch[4])), free, {k: "%.3g" % v for k, v in gaps.items()}))


if __name__ == "__main__":
    main()
