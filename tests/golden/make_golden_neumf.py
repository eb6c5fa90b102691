"""Golden NeuMF / MLP trace produced by the REFERENCE's own classes (model/general_recommender/NeuMF.py and MLP.py).

Both classes are loaded whole and unchanged with oracle/ref_models._load_file and run under oracle/tf_shim.py, as
make_golden_srgnn.py loads its class.  The ops they need beyond the shim's — layers.dense, layers.Dense, nn.relu — are
make_golden_caser.attach_caser_ops' (on top of make_golden_sasrec.attach_sasrec_ops and make_golden_gru4rec.attach_ops), by
their published definitions [EXT: tensorflow r1.12]; losses.sigmoid_cross_entropy and maximum are the shim's own.  check_ops() puts each of them on a
small hand-computed value before use.  `util.learner`, `util.tool`, `util.data_generator` and `util.data_iterator` are
the reference's own files; the recorded epoch draws from the reference's own PointwiseSampler (oracle/_ref).

    python tests/golden/make_golden_neumf.py              # needs the reference tree and oracle/_ref

Writes tests/golden/tfgraph_neumf.npz:
  shape, indptr, indices       the toy matrix (157 x 131)
  <case>_init_seed             the initial variables are neumf_restatement.init_tables(157, 131, d, layers, seed)
  <case>_users / _items / _labels    [steps, 20]: the fed batches.  Every batch holds a repeated user, a repeated item
                               and one fully repeated (user, item, label) instance
  <case>_loss_{f32,f64}        [steps] the loss fetched with each step (before its update)
  <case>_f64_<var>             the vectors, [steps, ...] float32: the variable after each step of the float64 run MINUS
                               its initial value
  <case>_q_<var>, _scale_<var> the matrices, [steps, ...] int16 and [steps]: the same difference in counts of the step's
                               scale (pack_tables)
  <case>_gap_<var>             [steps]: max |float32 run - float64 run| of the variable after each step
  epoch_*                      one train_model() epoch of `default` at batch_size 16 through a recording session with the
                               reference's PointwiseSampler under numpy and libc seed epoch_seed: epoch_users / _items / _labels
                               [S, 16] in the order fed (the last batch filled up with its first entry), epoch_rows [S]
                               the true sizes, the end tables under the case name `epoch`
  predict_users, predict_cand, predict_<case>_{f32,f64}, predict_cand_<case>_{f32,f64}
                               predict() after the last step of `odd` and of `default`, full mode and 3 candidates per
                               user, for 27 users
"""
import ctypes
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
import make_golden_gru4rec as G               # noqa: E402
import make_golden_caser as C                 # noqa: E402
import neumf_restatement as P                 # noqa: E402

B_STEP, B_EPOCH = 20, 16
EPOCH_SEED = 7311
FEED_SEED = 7312
N_PREDICT = 27


def load_class(name):
    """the reference module model/general_recommender/<name>.py, executed under the shim (oracle.ref_models.load, with
    the two util modules MLP.py imports besides)"""
    saved_tf = tf_shim.install()
    shadowed = rm._SHADOWED + ("util.data_generator", "util.data_iterator")
    saved = {k: sys.modules.get(k) for k in shadowed}
    try:
        util = types.ModuleType("util")
        util.__path__ = []
        sys.modules["util"] = util
        for sub in ("tool", "learner", "data_iterator", "data_generator"):
            setattr(util, sub, rm._load_file("util." + sub, os.path.join(rm.REF, "util", sub + ".py")))
        for fn in ("timer", "l2_loss", "inner_product", "log_loss", "csr_to_user_dict", "typeassert", "randint_choice",
                   "pad_sequences", "argmax_top_k"):
            setattr(util, fn, getattr(util.tool, fn))
        util.DataIterator = util.data_iterator.DataIterator
        util.Logger = rm.MemoryLogger
        data = types.ModuleType("data")
        data.PairwiseSampler = data.PointwiseSampler = rm.ReplaySampler
        sys.modules["data"] = data
        ev = types.ModuleType("evaluator")
        ev.ProxyEvaluator = rm.RecordingEvaluator
        sys.modules["evaluator"] = ev
        model_pkg = types.ModuleType("model")
        model_pkg.__path__ = []
        sys.modules["model"] = model_pkg
        rm._load_file("model.AbstractRecommender", os.path.join(rm.REF, "model", "AbstractRecommender.py"))
        mod = rm._load_file("model.general_recommender." + name,
                            os.path.join(rm.REF, "model", "general_recommender", name + ".py"))
        sys.modules.pop("model.general_recommender." + name, None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


def check_ops():
    """every op the two classes take from outside the shim's own set, and the two of the shim's the issue names, on a
    small hand-computed value"""
    tf = tf_shim
    run = lambda t: tf._evaluate([t], {})[0]
    tf.set_float("float64")
    tf.reset_default_graph()
    tf._GRAPH.collections = {}
    x = tf.constant(np.asarray([[1.0, -2.0], [0.5, 0.0]]))
    assert run(tf.nn.relu(x)).tolist() == [[1.0, 0.0], [0.5, 0.0]]
    assert run(tf.maximum(x, 0.25)).tolist() == [[1.0, 0.25], [0.5, 0.25]]
    # layers.dense: kernel [2, 3] then bias [3], relu(x kernel + bias)
    n0 = len(tf._GRAPH.variables)
    out = tf.layers.dense(x, units=3, activation=tf.nn.relu)
    kernel, bias = tf._GRAPH.variables[n0:]
    assert tuple(kernel.value.shape) == (2, 3) and tuple(bias.value.shape) == (3,) and not bias.numpy().any()
    assert np.abs(kernel.numpy()).max() <= np.sqrt(6.0 / 5.0)                # glorot uniform's limit
    kernel.load(np.asarray([[1.0, 0.0, -1.0], [0.0, 1.0, 1.0]]))
    bias.load(np.asarray([0.5, 0.5, 0.5]))
    assert run(out).tolist() == [[1.5, 0.0, 0.0], [1.0, 0.5, 0.0]]
    # layers.Dense: the variables are made at the first call, the second call shares them
    layer = tf.layers.Dense(units=1, activation=tf.nn.relu, name="layer0")
    n1 = len(tf._GRAPH.variables)
    a, b = layer(x), layer(tf.constant(np.asarray([[2.0, 2.0]])))
    assert len(tf._GRAPH.variables) == n1 + 2
    k1, b1 = tf._GRAPH.variables[n1:]
    k1.load(np.asarray([[1.0], [1.0]]))
    b1.load(np.asarray([0.25]))
    assert run(a).tolist() == [[0.0], [0.75]] and run(b).tolist() == [[4.25]]
    # losses.sigmoid_cross_entropy: the MEAN of max(z, 0) - z y + log(1 + exp(-|z|)); at z = 0 every term is log 2
    z = tf.constant(np.asarray([0.0, 0.0, np.log(3.0)]))
    y = tf.constant(np.asarray([1.0, 0.0, 1.0]))
    want = (2 * np.log(2.0) + np.log(4.0 / 3.0)) / 3.0
    assert abs(float(run(tf.losses.sigmoid_cross_entropy(y, z))) - want) < 1e-15
    tf._GRAPH.collections = {}
    tf.reset_default_graph()
    return True


def build(name, dataset, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    tf_shim._GRAPH.collections = {}
    mod = load_class(name)
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = name
    conf.update(hyper)
    sess = G.RecordingSession(seed=0)
    model = getattr(mod, name)(sess, dataset, conf)
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess, mod


def _hyper(case, batch):
    model, layers, d, loss, learner, reg_mf, reg_mlp, _ = P.CASES[case]
    out = dict(layers=list(layers), reg_mlp=reg_mlp, learning_rate=P.LR, learner=learner, is_pairwise=False, num_neg=4,
               loss_function=loss, epochs=1, batch_size=batch, verbose=1, init_method="normal", stddev=0.01)
    if model == "NeuMF":
        out.update(embedding_size=d, reg_mf=reg_mf, mf_pretrain="pretrain/GMF", mlp_pretrain="pretrain/MLP")
    return model, out


def _variables(case, U, I):
    _, layers, d = P.CASES[case][:3]
    want = P.shapes(U, I, d, layers)
    variables = list(tf_shim._GRAPH.variables)
    assert len(variables) == len(want), (len(variables), list(want))
    for v, (name, shape) in zip(variables, want.items()):
        assert tuple(v.value.shape) == shape, (name, tuple(v.value.shape), shape)
    return variables, list(want)


def make_batches(R, steps, seed):
    """steps x B_STEP instances: 17 drawn (train pairs with label 1, other pairs with label 0), then a second item for
    the user of slot 0, a second user for the item of slot 1 and a whole copy of slot 2; the order shuffled"""
    rs = np.random.RandomState(seed)
    U, I = R.shape
    coo = R.tocoo()
    dense = np.asarray(R.todense()) > 0
    out = []
    for _ in range(steps):
        users, items, labels = [], [], []
        for k in range(B_STEP - 3):
            if rs.rand() < 0.4:
                j = rs.randint(len(coo.row))
                users.append(int(coo.row[j])), items.append(int(coo.col[j])), labels.append(1.0)
            else:
                u = rs.randint(U)
                i = rs.randint(I)
                while dense[u, i]:
                    i = rs.randint(I)
                users.append(u), items.append(i), labels.append(0.0)
        users.append(users[0]), items.append((items[0] + 1 + rs.randint(I - 1)) % I), labels.append(0.0)
        users.append((users[1] + 1 + rs.randint(U - 1)) % U), items.append(items[1]), labels.append(0.0)
        users.append(users[2]), items.append(items[2]), labels.append(labels[2])
        order = rs.permutation(B_STEP)
        u, i, y = (np.asarray(a)[order] for a in (users, items, labels))
        assert len(set(zip(u.tolist(), i.tolist(), y.tolist()))) < B_STEP
        assert len(set(u.tolist())) < B_STEP - 1 and len(set(i.tolist())) < B_STEP - 1
        out.append((u.astype(np.int32), i.astype(np.int32), y.astype(np.float32)))
    return out


def _tabs(variables):
    return [v.numpy() for v in variables]


def run_case(ds, case, init, batches, with_predict=None):
    U, I = ds.train_matrix.shape
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        name, hyper = _hyper(case, B_STEP)
        model, sess, _ = build(name, ds, hyper, width)
        variables, names = _variables(case, U, I)
        for var, n in zip(variables, names):
            var.load(init[n])
        tabs, losses = [], []
        for users, items, labels in batches:
            feed = {model.user_input: users.tolist(), model.item_input: items.tolist(), model.labels: labels.tolist()}
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=feed)
            losses.append(float(loss))
            tabs.append(_tabs(variables))
        out[tag] = (tabs, losses)
        if with_predict is not None:
            users, cand = with_predict
            out[tag + "_predict"] = _np(np.stack(model.predict(list(users), None)), width)
            out[tag + "_predict_cand"] = _np(np.stack(model.predict(list(users), [list(c) for c in cand])), width)
    return out, names


def pack_tables(case, names, tabs_by_tag, init):
    """the f64 trace as differences from the initial values.  The vectors (biases) as float32, exact to 2^-24 of the
    difference; so are matrices that moved too far for the counts below (the epoch's end tables).  The matrices as int16 counts of each step's own scale max|difference| / 32767 — float32 differences of
    every case would take the file past the size limit.  Their round trip is within max|difference| / 65000 and,
    asserted here, within 1e-6 max|value|: a tenth of the 1e-5 max|want| that reads it, spent out of the device's
    margin, not added to it.  Of the f32 twin only what the tests read: its distance from the f64 trace per step and
    variable"""
    out = {}
    for j, name in enumerate(names):
        i64 = init[name].astype(np.float64)
        want = np.stack([t[j] for t in tabs_by_tag["f64"]]).astype(np.float64)
        delta = want - i64[None]
        scale = np.abs(delta).reshape(len(delta), -1).max(axis=1, initial=0) / 32767.0
        coarse = (scale * 32767.0 / 65000.0 > 1e-6 * np.abs(want).reshape(len(want), -1).max(axis=1, initial=0)).any()
        if init[name].ndim == 1 or init[name].size == 0 or coarse:
            back = i64[None] + delta.astype(np.float32).astype(np.float64)
            assert np.abs(back - want).max(initial=0) <= 2.0 ** -24 * np.abs(delta).max(initial=0)
            out["%s_f64_%s" % (case, name)] = delta.astype(np.float32)
        else:
            safe = np.where(scale > 0, scale, 1.0).reshape((-1,) + (1,) * (delta.ndim - 1))
            q = np.rint(delta / safe).astype(np.int16)
            back = i64[None] + q.astype(np.float64) * safe
            lost = np.abs(back - want).reshape(len(want), -1).max(axis=1)
            assert (lost <= np.abs(delta).reshape(len(want), -1).max(axis=1) / 65000.0).all()
            assert (lost <= 1e-6 * np.abs(want).reshape(len(want), -1).max(axis=1)).all(), name
            out["%s_q_%s" % (case, name)] = q
            out["%s_scale_%s" % (case, name)] = np.where(scale > 0, scale, 1.0)
        twin = np.stack([t[j] for t in tabs_by_tag["f32"]]).astype(np.float64)
        out["%s_gap_%s" % (case, name)] = np.abs(twin - want).reshape(len(want), -1).max(axis=1, initial=0)
    return out


def run_epoch(ds, init):
    """one whole train_model() of `default` at batch 16 with the reference's own PointwiseSampler"""
    from oracle import ref
    smod = ref.sampler_module()
    assert smod is not None, "oracle/_ref is not built (python -c 'import oracle; oracle.build()')"
    U, I = ds.train_matrix.shape
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        name, hyper = _hyper(P.EPOCH_CASE, B_EPOCH)
        model, sess, mod = build(name, ds, hyper, width)
        # the sampler's negatives come from libc rand() (util/cython/random_choice.pyx), which numpy's seed does not
        # reach: it is seeded here as well, and the second width replays the batches the first one was fed
        if "f32" not in out and "f64" not in out:
            mod.PointwiseSampler = smod.PointwiseSampler
            ctypes.CDLL(None).srand(EPOCH_SEED)
        else:
            mod.PointwiseSampler = rm.ReplaySampler
            rm.ReplaySampler.batches = list(out[WIDTHS[0][0]]["batches"])
        variables, names = _variables(P.EPOCH_CASE, U, I)
        for var, n in zip(variables, names):
            var.load(init[n])
        np.random.seed(EPOCH_SEED)
        sess.feed_log = []
        model.train_model()
        fed = [f for f in sess.feed_log if len(f) == 3]           # predict() feeds two placeholders
        sess.feed_log = None
        keys = sorted(fed[0])
        ku = [k for k in keys if "user" in k][0]
        ki = [k for k in keys if "item" in k][0]
        kl = [k for k in keys if "label" in k][0]
        out[tag] = dict(batches=[(np.asarray(f[ku], np.int32), np.asarray(f[ki], np.int32),
                                  np.asarray(f[kl], np.float32)) for f in fed], tabs=[_tabs(variables)])
    a, b = out["f32"]["batches"], out["f64"]["batches"]
    assert len(a) == len(b) and all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))
    return out, names


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    G.attach_ops()                              # make_golden_caser's own checks read its gather
    C.attach_caser_ops()
    check_ops()
    R = toy_matrix(isolated=False)
    U, I = R.shape
    ds = rm.Dataset(R)
    out = dict(shape=np.asarray(R.shape, np.int64), indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32),
               lr=np.float64(P.LR), cases=np.asarray(sorted(P.CASES)), batch_step=np.int64(B_STEP),
               batch_epoch=np.int64(B_EPOCH))
    rs = np.random.RandomState(7)
    predict_users = np.sort(rs.choice(U, N_PREDICT, replace=False)).astype(np.int32)
    cand = rs.randint(0, I, (N_PREDICT, 3)).astype(np.int32)
    cand[0] = [3, 0, I - 1]
    out.update(predict_users=predict_users, predict_cand=cand)
    gaps = {}
    for k, case in enumerate(sorted(P.CASES)):
        _, layers, d, _, _, _, _, steps = P.CASES[case]
        init = P.init_tables(U, I, d, layers, seed=900 + k)
        batches = make_batches(R, steps, FEED_SEED + k)
        res, names = run_case(ds, case, init, batches, (predict_users, cand) if case in P.PREDICT_CASES else None)
        out["%s_init_seed" % case] = np.int64(900 + k)
        out["%s_users" % case] = np.stack([b[0] for b in batches])
        out["%s_items" % case] = np.stack([b[1] for b in batches])
        out["%s_labels" % case] = np.stack([b[2] for b in batches])
        for tag, _ in WIDTHS:
            out["%s_loss_%s" % (case, tag)] = np.asarray(res[tag][1], np.float64)
        out.update(pack_tables(case, names, {tag: res[tag][0] for tag, _ in WIDTHS}, init))
        if case in P.PREDICT_CASES:
            for tag, _ in WIDTHS:
                out["predict_%s_%s" % (case, tag)] = res[tag + "_predict"]
                out["predict_cand_%s_%s" % (case, tag)] = res[tag + "_predict_cand"]
        gaps[case] = max(out["%s_gap_%s" % (case, n)].max(initial=0) for n in names)
    # one whole epoch of train_model()
    _, layers, d = P.CASES[P.EPOCH_CASE][:3]
    init = P.init_tables(U, I, d, layers, seed=990)
    ep, names = run_epoch(ds, init)
    batches = ep["f64"]["batches"]
    S = len(batches)
    rows = np.asarray([len(b[0]) for b in batches], np.int64)
    assert (rows[:-1] == B_EPOCH).all() and 1 <= rows[-1] <= B_EPOCH and rows.sum() == R.nnz * 5

    def filled(j, dtype):
        a = np.zeros((S, B_EPOCH), dtype)
        for s, b in enumerate(batches):
            a[s] = b[j][0]
            a[s, :len(b[j])] = b[j]
        return a
    out.update(epoch_users=filled(0, np.int32), epoch_items=filled(1, np.int32), epoch_labels=filled(2, np.float32),
               epoch_rows=rows, epoch_seed=np.int64(EPOCH_SEED), epoch_init_seed=np.int64(990))
    out.update(pack_tables("epoch", names, {tag: ep[tag]["tabs"] for tag, _ in WIDTHS}, init))
    gaps["epoch"] = max(out["epoch_gap_%s" % n].max(initial=0) for n in names)
    path = os.path.join(HERE, "tfgraph_neumf.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); %d epoch steps; fp32 vs fp64 table gaps %s; predict gaps %s" % (
        path, os.path.getsize(path), S, {k: "%.3g" % v for k, v in gaps.items()},
        {c: "%.3g" % np.abs(out["predict_%s_f32" % c] - out["predict_%s_f64" % c]).max() for c in P.PREDICT_CASES}))


if __name__ == "__main__":
    main()
