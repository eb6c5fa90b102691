"""Golden ConvNCF trace produced by the REFERENCE's own class (model/general_recommender/ConvNCF.py).

The class is loaded whole and unchanged (make_golden_neumf.load_class) and run under oracle/tf_shim.py.  The ops it needs
beyond the shim's are attached here by their published definitions [EXT: tensorflow r1.12] and put on small hand-computed
values by check_ops() before use:
  nn.conv2d          NHWC input, HWIO filter, strides [1, s, s, 1]; SAME pads max((ceil(n / s) - 1) s + k - n, 0) in all,
                     the smaller half in front (nothing at all for a 2x2 filter at stride 2 over even sizes)
  constant           honours shape=: a scalar fills the shape (the shim's own drops it; a conv bias made from it would be
                     a scalar and receive the SUM of the per-channel gradients)
  gradients, Optimizer.apply_gradients, group
                     ConvNCF.py:138-145 takes tf.gradients(opt_loss, vars) once and hands the halves to two
                     AdagradOptimizers; grouped, that is one minimisation of opt_loss in which each variable is moved by
                     the optimizer it was handed to — one shim _Minimize whose Adagrad picks lr_embed or lr_net per variable
  reshape            make_golden_gru4rec.attach_ops'
The batched matmul of the outer product is the shim's own (`x @ y` on [n, d, 1] and [n, 1, d]), checked here as well.
`util.learner`, `util.tool` are the reference's own files; the recorded epoch draws from the reference's own
PairwiseSampler (oracle/_ref).

    python tests/golden/make_golden_convncf.py              # needs the reference tree and oracle/_ref

Writes tests/golden/tfgraph_convncf.npz, in the layout of tfgraph_neumf.npz:
  shape, indptr, indices       the toy matrix (157 x 131)
  <case>_init_seed             the initial variables are convncf_restatement.init_tables(157, 131, d, net_channel, seed)
  <case>_users / _pos / _neg   [steps, 20]: the fed triplets.  Every batch holds a repeated user, an item that is positive in
                               one triplet and negative in another, and one triplet given twice
  <case>_loss_{f32,f64}        [steps] self.loss fetched with each step (before its update, without the regularisers)
  <case>_f64_<var>             the vectors, [steps, ...] float32: the variable after each step of the float64 run MINUS its
                               initial value
  <case>_q_<var>, _scale_<var> the matrices and kernels, [steps, ...] int16 and [steps]: the same difference in counts of
                               the step's scale (make_golden_neumf.pack_tables)
  <case>_gap_<var>             [steps]: max |float32 run - float64 run| of the variable after each step
  epoch_*                      one train_model() epoch of `hinge` at batch_size 16 with the reference's PairwiseSampler
                               under numpy and libc seed epoch_seed: epoch_users / _pos / _neg [S, 16] in the order fed (the
                               last batch filled up with its first entry), epoch_rows [S] the true sizes, the end tables
                               under the case name `epoch`, epoch_log the lines train_model() logged
  predict_users, predict_cand, predict_<case>_{f32,f64}, predict_cand_<case>_{f32,f64}
                               predict() after the last step of `regs` and of `square`, full mode and 3 candidates per
                               user, for 27 users
"""
import ctypes
import os
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
import make_golden_gru4rec as G               # noqa: E402
import make_golden_neumf as N                 # noqa: E402
import convncf_restatement as P               # noqa: E402

B_STEP, B_EPOCH = 20, 16
EPOCH_SEED = 7411
FEED_SEED = 7412
N_PREDICT = 27


# ------------------------------------------------------------------ the ops ConvNCF.py needs beyond the shim's
class _Gradient:
    """one entry of tf.gradients(loss, xs): d loss / d var, taken when the grouped applications run"""

    def __init__(self, loss, var):
        self.loss, self.var = loss, var


class _Apply:
    """Optimizer.apply_gradients(zip(grads, vars)) before it is grouped"""

    def __init__(self, opt, pairs):
        self.opt, self.pairs = opt, pairs


class _PerVariable(tf_shim._Optimizer):
    """the grouped applications as one optimiser: every variable is moved by the optimizer it was handed to"""

    def __init__(self, applies):
        self.by_var = {id(v): a.opt for a in applies for _, v in a.pairs}
        self.opts = [a.opt for a in applies]

    def slots(self, var):
        return self.by_var[id(var)].slots(var)

    def begin(self, dt):
        for opt in self.opts:
            opt.begin(dt)

    def update(self, var, st, g, sparse, rows):
        self.by_var[id(var)].update(var, st, g, sparse, rows)

    def finish(self):
        for opt in self.opts:
            opt.finish()


def attach_convncf_ops():
    import torch
    import torch.nn.functional as F
    T = tf_shim.Tensor
    G.attach_ops()

    def conv2d(input, filter, strides, padding, name=None, **_):   # noqa: A002
        strides = [int(s) for s in strides]
        assert strides[0] == 1 and strides[3] == 1 and padding in ("SAME", "VALID")

        def f(a, k):
            x, w = a.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1)
            if padding == "SAME":
                pads = []
                for n, size, s in ((x.shape[3], w.shape[3], strides[2]), (x.shape[2], w.shape[2], strides[1])):
                    total = max((-(-n // s) - 1) * s + size - n, 0)
                    pads += [total // 2, total - total // 2]
                x = F.pad(x, pads)
            return F.conv2d(x, w, stride=(strides[1], strides[2])).permute(0, 2, 3, 1)
        return T(f, [input, filter])

    def constant(value, dtype=None, shape=None, name=None, **_):
        a = np.asarray(value)
        if shape is not None:
            a = np.broadcast_to(a, [int(s) for s in shape]).copy()
        return tf_shim._Const(a)

    def gradients(ys, xs, **_):
        return [_Gradient(ys, x) for x in xs]

    def apply_gradients(self, grads_and_vars, global_step=None, name=None):
        pairs = list(grads_and_vars)
        assert all(isinstance(g, _Gradient) and g.var is v for g, v in pairs)
        return _Apply(self, pairs)

    def group(*ops, **_):
        assert ops and all(isinstance(op, _Apply) for op in ops)
        losses = {id(g.loss) for op in ops for g, _ in op.pairs}
        assert len(losses) == 1
        opt = _PerVariable(ops)
        mz = tf_shim._Minimize(opt, ops[0].pairs[0][0].loss)
        assert {id(v) for v in mz.vars} == set(opt.by_var)         # every handed variable is reached, and no other
        return mz

    tf_shim.nn.conv2d, tf_shim.constant, tf_shim.gradients, tf_shim.group = conv2d, constant, gradients, group
    tf_shim._Optimizer.apply_gradients = apply_gradients
    return check_ops()


def check_ops():
    """every attached op, and the shim's batched matmul, on a small hand-computed value"""
    tf = tf_shim
    run = lambda t: tf._evaluate([t], {})[0]
    tf.set_float("float64")
    tf.reset_default_graph()
    tf._GRAPH.collections = {}
    # conv2d, stride 2, SAME on even sizes: channel 0 weighs the patch [[1, 2], [3, 4]], channel 1 picks corner (0, 0)
    x = tf.constant(np.arange(16.0).reshape(1, 4, 4, 1))
    k = np.zeros((2, 2, 1, 2))
    k[:, :, 0, 0] = [[1.0, 2.0], [3.0, 4.0]]
    k[0, 0, 0, 1] = 1.0
    out = run(tf.nn.conv2d(x, tf.constant(k), strides=[1, 2, 2, 1], padding="SAME"))
    assert tuple(out.shape) == (1, 2, 2, 2)
    assert out[0, :, :, 0].tolist() == [[34.0, 54.0], [114.0, 134.0]] and out[0, :, :, 1].tolist() == [[0.0, 2.0], [8.0, 10.0]]
    # the two axes are not transposed: corner (0, 1) is one COLUMN to the right
    k2 = np.zeros((2, 2, 1, 1))
    k2[0, 1, 0, 0] = 1.0
    out = run(tf.nn.conv2d(x, tf.constant(k2), strides=[1, 2, 2, 1], padding="SAME"))
    assert out[0, :, :, 0].tolist() == [[1.0, 3.0], [9.0, 11.0]]
    # SAME on an odd size pads one row and column behind: ceil(3 / 2) = 2 positions a side
    ones = tf.constant(np.ones((1, 3, 3, 1)))
    out = run(tf.nn.conv2d(ones, tf.constant(np.ones((2, 2, 1, 1))), strides=[1, 2, 2, 1], padding="SAME"))
    assert out[0, :, :, 0].tolist() == [[4.0, 2.0], [2.0, 1.0]]
    # two input channels: the channel is the third axis of the filter
    x2 = tf.constant(np.stack([np.ones((2, 2)), 2 * np.ones((2, 2))], axis=-1)[None])
    k3 = np.zeros((2, 2, 2, 1))
    k3[1, 1, 0, 0], k3[0, 0, 1, 0] = 1.0, 10.0
    assert run(tf.nn.conv2d(x2, tf.constant(k3), strides=[1, 2, 2, 1], padding="SAME")).reshape(-1).tolist() == [21.0]
    # constant with a shape
    c = run(tf.constant(0.1, shape=[3]))
    assert tuple(c.shape) == (3,) and c.tolist() == [0.1, 0.1, 0.1]
    assert tuple(tf.Variable(tf.constant(0.1, shape=[3])).value.shape) == (3,)
    # the batched matmul of the outer product
    p = tf.constant(np.asarray([[1.0, 2.0], [3.0, 4.0]]))
    q = tf.constant(np.asarray([[5.0, 6.0], [7.0, 8.0]]))
    e = run(tf.matmul(tf.expand_dims(p, 2), tf.expand_dims(q, 1)))
    assert e.tolist() == [[[5.0, 6.0], [10.0, 12.0]], [[21.0, 24.0], [28.0, 32.0]]]
    # gradients + two apply_gradients + group: loss = sum(v[[1, 1]] * w): dv = [0, 2 w] = [0, 6] (sparse: row 0 and its
    # accumulator stay), dw = 2 v[1] = 4; Adagrad from 0.1 with its own learning rate per variable
    v = tf.Variable(np.asarray([1.0, 2.0]), name="v")
    w = tf.Variable(np.asarray([3.0]), name="w")
    loss = tf.reduce_sum(tf.nn.embedding_lookup(v, tf.constant(np.asarray([1, 1]))) * w)
    grads = tf.gradients(loss, [v, w])
    op = tf.group(tf.train.AdagradOptimizer(0.5).apply_gradients(zip(grads[:1], [v])),
                  tf.train.AdagradOptimizer(0.25).apply_gradients(zip(grads[1:], [w])))
    sess = tf.Session()
    got, _ = sess.run((loss, op))
    assert float(got) == 12.0
    assert v.numpy().tolist() == [1.0, 2.0 - 0.5 * 6.0 * (1.0 / np.sqrt(36.1))]
    assert w.numpy().tolist() == [3.0 - 0.25 * 4.0 * (1.0 / np.sqrt(16.1))]
    assert op.state[id(v)]["accum"].tolist() == [0.1, 36.1] and op.state[id(w)]["accum"].tolist() == [16.1]
    tf._GRAPH.collections = {}
    tf.reset_default_graph()
    return True


def build(dataset, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    tf_shim._GRAPH.collections = {}
    mod = N.load_class("ConvNCF")
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "ConvNCF"
    conf.update(hyper)
    sess = G.RecordingSession(seed=0)
    model = mod.ConvNCF(sess, dataset, conf)
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess, mod


def _hyper(case, batch):
    d, channels, loss, regs, lr_embed, lr_net, _ = P.CASES[case]
    return dict(epochs=1, batch_size=batch, embedding_size=d, regs=list(regs), net_channel=list(channels),
                lr_embed=lr_embed, lr_net=lr_net, num_negatives=4, loss_function=loss, keep=1.0,
                embed_init_method="tnormal", weight_init_method="xavier_normal", stddev=0.01, verbose=1)


def _variables(case, U, I):
    d, channels = P.CASES[case][:2]
    want = P.shapes(U, I, d, channels)
    variables = list(tf_shim._GRAPH.variables)
    assert len(variables) == len(want) and list(want) == P.names(len(channels)), (len(variables), list(want))
    for v, (name, shape) in zip(variables, want.items()):
        assert tuple(v.value.shape) == shape, (name, tuple(v.value.shape), shape)
    return variables, list(want)


def make_batches(R, steps, seed):
    """steps x B_STEP triplets: 17 drawn from the train pairs with a negative outside the user's row, then a second
    triplet for the user of slot 0, a triplet whose NEGATIVE is the positive of slot 1, and a whole copy of slot 2; the
    order shuffled"""
    rs = np.random.RandomState(seed)
    U, I = R.shape
    coo = R.tocoo()
    dense = np.asarray(R.todense()) > 0

    def negative(u):
        j = rs.randint(I)
        while dense[u, j]:
            j = rs.randint(I)
        return j
    out = []
    for _ in range(steps):
        users, pos, neg = [], [], []
        for k in range(B_STEP - 3):
            j = rs.randint(len(coo.row))
            users.append(int(coo.row[j])), pos.append(int(coo.col[j])), neg.append(negative(int(coo.row[j])))
        users.append(users[0]), pos.append(pos[0]), neg.append(negative(users[0]))
        others = [j for j in range(len(coo.row)) if not dense[coo.row[j], pos[1]]]
        j = others[rs.randint(len(others))]
        users.append(int(coo.row[j])), pos.append(int(coo.col[j])), neg.append(pos[1])
        users.append(users[2]), pos.append(pos[2]), neg.append(neg[2])
        order = rs.permutation(B_STEP)
        u, i, j = (np.asarray(a)[order].astype(np.int32) for a in (users, pos, neg))
        assert len(set(zip(u.tolist(), i.tolist(), j.tolist()))) < B_STEP and len(set(u.tolist())) < B_STEP - 1
        assert set(i.tolist()) & set(j.tolist())
        out.append((u, i, j))
    return out


def _tabs(variables):
    return [v.numpy() for v in variables]


def _feed(model, users, pos, neg):
    return {model.user_input: users.tolist(), model.item_input_pos: pos.tolist(), model.item_input_neg: neg.tolist()}


def run_case(ds, case, init, batches, with_predict=None):
    U, I = ds.train_matrix.shape
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess, _ = build(ds, _hyper(case, B_STEP), width)
        assert "load pretrained params unsuccessful!" in "\n".join(rm.MemoryLogger.lines)
        variables, names = _variables(case, U, I)
        for var, n in zip(variables, names):
            var.load(init[n])
        tabs, losses = [], []
        for users, pos, neg in batches:
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=_feed(model, users, pos, neg))
            losses.append(float(loss))
            tabs.append(_tabs(variables))
        out[tag] = (tabs, losses)
        if with_predict is not None:
            users, cand = with_predict
            full = np.stack(model.predict(list(users), None))
            cands = np.stack(model.predict(list(users), [list(c) for c in cand]))
            assert full.shape == (len(users), I, 1) and cands.shape == (len(users), 3, 1)
            out[tag + "_predict"] = _np(full[..., 0], width)
            out[tag + "_predict_cand"] = _np(cands[..., 0], width)
    return out, names


def run_epoch(ds, init):
    """one whole train_model() of EPOCH_CASE at batch 16 with the reference's own PairwiseSampler"""
    from oracle import ref
    smod = ref.sampler_module()
    assert smod is not None, "oracle/_ref is not built (python -c 'import oracle; oracle.build()')"
    U, I = ds.train_matrix.shape
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess, mod = build(ds, _hyper(P.EPOCH_CASE, B_EPOCH), width)
        # the sampler's negatives come from libc rand() (util/cython/random_choice.pyx), which numpy's seed does not
        # reach: it is seeded here as well, and the second width replays the batches the first one was fed
        if not out:
            mod.PairwiseSampler = smod.PairwiseSampler
            ctypes.CDLL(None).srand(EPOCH_SEED)
        else:
            mod.PairwiseSampler = rm.ReplaySampler
            rm.ReplaySampler.batches = list(out[WIDTHS[0][0]]["batches"])
        variables, names = _variables(P.EPOCH_CASE, U, I)
        for var, n in zip(variables, names):
            var.load(init[n])
        np.random.seed(EPOCH_SEED)
        sess.feed_log = []
        model.train_model()
        fed = [f for f in sess.feed_log if len(f) == 3]           # predict() feeds two placeholders
        sess.feed_log = None
        out[tag] = dict(batches=[(np.asarray(f["user_input"], np.int32), np.asarray(f["item_input_pos"], np.int32),
                                  np.asarray(f["item_input_neg"], np.int32)) for f in fed], tabs=[_tabs(variables)],
                        log=list(rm.MemoryLogger.lines))
    a, b = out["f32"]["batches"], out["f64"]["batches"]
    assert len(a) == len(b) and all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))
    return out, names


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_convncf_ops()
    R = toy_matrix(isolated=False)
    U, I = R.shape
    ds = rm.Dataset(R)
    out = dict(shape=np.asarray(R.shape, np.int64), indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32),
               cases=np.asarray(sorted(P.CASES)), batch_step=np.int64(B_STEP), batch_epoch=np.int64(B_EPOCH))
    rs = np.random.RandomState(7)
    predict_users = np.sort(rs.choice(U, N_PREDICT, replace=False)).astype(np.int32)
    cand = rs.randint(0, I, (N_PREDICT, 3)).astype(np.int32)
    cand[0] = [3, 0, I - 1]
    out.update(predict_users=predict_users, predict_cand=cand)
    gaps = {}
    for k, case in enumerate(sorted(P.CASES)):
        d, channels, steps = P.CASES[case][0], P.CASES[case][1], P.CASES[case][6]
        init = P.init_tables(U, I, d, channels, seed=1100 + k)
        batches = make_batches(R, steps, FEED_SEED + k)
        res, names = run_case(ds, case, init, batches, (predict_users, cand) if case in P.PREDICT_CASES else None)
        out["%s_init_seed" % case] = np.int64(1100 + k)
        for j, what in enumerate(("users", "pos", "neg")):
            out["%s_%s" % (case, what)] = np.stack([b[j] for b in batches])
        for tag, _ in WIDTHS:
            out["%s_loss_%s" % (case, tag)] = np.asarray(res[tag][1], np.float64)
        out.update(N.pack_tables(case, names, {tag: res[tag][0] for tag, _ in WIDTHS}, init))
        if case in P.PREDICT_CASES:
            for tag, _ in WIDTHS:
                out["predict_%s_%s" % (case, tag)] = res[tag + "_predict"]
                out["predict_cand_%s_%s" % (case, tag)] = res[tag + "_predict_cand"]
        gaps[case] = max(out["%s_gap_%s" % (case, n)].max(initial=0) for n in names)
    # one whole epoch of train_model()
    d, channels = P.CASES[P.EPOCH_CASE][:2]
    init = P.init_tables(U, I, d, channels, seed=1190)
    ep, names = run_epoch(ds, init)
    batches = ep["f64"]["batches"]
    S = len(batches)
    rows = np.asarray([len(b[0]) for b in batches], np.int64)
    assert (rows[:-1] == B_EPOCH).all() and 1 <= rows[-1] <= B_EPOCH and rows.sum() == R.nnz

    def filled(j):
        a = np.zeros((S, B_EPOCH), np.int32)
        for s, b in enumerate(batches):
            a[s] = b[j][0]
            a[s, :len(b[j])] = b[j]
        return a
    out.update(epoch_users=filled(0), epoch_pos=filled(1), epoch_neg=filled(2), epoch_rows=rows,
               epoch_seed=np.int64(EPOCH_SEED), epoch_init_seed=np.int64(1190), epoch_log=np.asarray(ep["f64"]["log"]))
    out.update(N.pack_tables("epoch", names, {tag: ep[tag]["tabs"] for tag, _ in WIDTHS}, init))
    gaps["epoch"] = max(out["epoch_gap_%s" % n].max(initial=0) for n in names)
    path = os.path.join(HERE, "tfgraph_convncf.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); %d epoch steps; fp32 vs fp64 table gaps %s; predict gaps %s" % (
        path, os.path.getsize(path), S, {k: "%.3g" % v for k, v in gaps.items()},
        {c: "%.3g" % np.abs(out["predict_%s_f32" % c] - out["predict_%s_f64" % c]).max() for c in P.PREDICT_CASES}))


if __name__ == "__main__":
    main()
