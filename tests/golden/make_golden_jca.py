"""Golden JCA trace produced by the REFERENCE's own class (model/general_recommender/JCA.py).

The class is loaded whole and unchanged (oracle.ref_models.load) and run under oracle/tf_shim.py.  The two ops it needs
beyond the shim's are attached here by their published definitions [EXT: tensorflow r1.12] and put on a small
hand-computed value first (check_ops): gather_nd, and zeros over a fetched length (`tf.zeros(tf.shape(x)[0])`).  The
shim's own maximum, identity, nn.relu and nn.elu are checked on a value as well.  Nothing under oracle/ changes.

    python tests/golden/make_golden_jca.py              # needs the reference tree

Writes tests/golden/tfgraph_jca.npz:
  shape, indptr, indices       the toy matrix (157 x 131)
  <case>_init_seed             the initial variables are jca_restatement.init_tables(157, 131, H, seed)
  <case>_rows_<s>, _cols_<s>   the block of step s (users, items); _p_<s>, _n_<s> [n, 2] the pairs as the class built them
                               (pairwise_neg_sampling under numpy seed <case>_pair_seed + s)
  <case>_loss_{f32,f64} [S]    the cost of each step (before its update)
  <case>_f64_<var> [S, ...]    the variable after each step of the float64 run MINUS its initial value
  <case>_gap_<var> [S]         max |float32 run - float64 run| of the variable after each step
  predict_users, predict_cand, predict_<case>_{f32,f64} [27, 131], predict_<case>_cand_{f32,f64} [27, 3]
                               evaluate() then predict() after the last step for 27 users, in full mode and with
                               recorded candidates
  epoch_*                      one train_model() epoch of `default` at batch_size 48 under numpy seed epoch_seed through
                               the recording session: per block s (4 x 3 of them, row batches outermost) the fed rows,
                               columns and pairs, its cost in both widths, the logged loss, the end tables under the case
                               name `epoch`.  The step case `default` runs at H = 33 and the epoch at the reference's
                               H = 50, so that the file stays within the size of a committed file
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
import jca_restatement as R                   # noqa: E402

STEPS = 3
EPOCH_SEED = 4148
N_PREDICT = 27
BLOCK = (40, 50)                              # block rows x block columns of the step cases: Bu != Bi


# ------------------------------------------------------------------ the ops the shim lacks
def attach_jca_ops():
    import torch
    T = tf_shim.Tensor
    if getattr(tf_shim.zeros, "jca", False):
        return
    shim_zeros = tf_shim.zeros

    def gather_nd(params, indices, name=None):
        """array_ops.gather_nd: out[...] = params[indices[..., 0], ..., indices[..., K - 1]]"""
        def f(p, idx):
            idx = idx.to(torch.int64)
            return p[tuple(idx[..., k] for k in range(idx.shape[-1]))]
        return T(f, [params, indices])

    def zeros(shape, dtype=None, **kw):
        """array_ops.zeros with a fetched scalar as the shape: a vector of that length"""
        if isinstance(shape, T):
            return T(lambda n: torch.zeros(int(n), dtype=tf_shim.float_dtype()), [shape])
        return shim_zeros(shape, dtype, **kw)
    zeros.jca = True

    tf_shim.gather_nd = gather_nd
    tf_shim.zeros = zeros


def check_ops():
    """every attached op, and the shim's ops the class had not used before, on a small hand-computed value"""
    tf = tf_shim
    tf.set_float("float64")
    tf.reset_default_graph()
    sess = tf.Session(seed=0)
    p = tf.constant(np.asarray([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]))
    assert sess.run(tf.gather_nd(p, tf.constant(np.asarray([[1, 2], [0, 0]])))).tolist() == [6.0, 1.0]
    assert sess.run(tf.gather_nd(p, tf.constant(np.asarray([[1], [1], [0]])))).tolist() == \
        [[4.0, 5.0, 6.0], [4.0, 5.0, 6.0], [1.0, 2.0, 3.0]]
    x = tf.constant(np.asarray([-1.0, 0.5, 2.0]))
    z = tf.zeros(tf.shape(x)[0])
    assert sess.run(z).tolist() == [0.0, 0.0, 0.0]
    assert sess.run(tf.maximum(x, z)).tolist() == [0.0, 0.5, 2.0]
    assert sess.run(tf.identity(x)).tolist() == [-1.0, 0.5, 2.0]
    assert sess.run(tf.nn.relu(x)).tolist() == [0.0, 0.5, 2.0]
    got = sess.run(tf.nn.elu(x))
    assert abs(got[0] - (np.exp(-1.0) - 1.0)) < 1e-15 and got[1:].tolist() == [0.5, 2.0]
    tf.reset_default_graph()
    return True


# ------------------------------------------------------------------ the class
def _hyper(case, batch, epochs=1, H=None):
    f, g, learner, reg, num_neg, H0, margin, lr = R.CASES[case]
    H = H0 if H is None else H
    return dict(hidden_neuron=H, learning_rate=lr, learner=learner, reg=reg, epochs=epochs, batch_size=batch, verbose=1,
                f_act=f, g_act=g, margin=margin, corruption_level=0.2, init_method="tnormal", stddev=0.01,
                num_neg=num_neg)


def build(ds, hyper, width, init):
    attach_jca_ops()
    model, sess, _ = rm.build("JCA", ds, hyper, width)
    variables = list(tf_shim._GRAPH.variables)
    U, I = ds.train_matrix.shape
    want = R.shapes(U, I, hyper["hidden_neuron"])
    assert [tuple(v.value.shape) for v in variables] == [want[k] for k in R.NAMES]
    for var, k in zip(variables, R.NAMES):
        var.load(init[k])
    return model, sess, variables


def feed_of(model, rows, cols, p, n):
    """the feed the class builds in train_model (JCA.py:148-159)"""
    return {model.input_R_U: model.train_R[rows, :], model.input_R_I: model.train_R[:, cols],
            model.input_OH_I: model.I_OH_mat[cols, :], model.input_P_cor: p, model.input_N_cor: n,
            model.row_idx: np.reshape(rows, (len(rows), 1)), model.col_idx: np.reshape(cols, (len(cols), 1))}


def make_blocks(Rm, case, seed):
    """per step (rows, cols): the first holds the row without an entry (user 5) and the hub column (item 0)"""
    rs = np.random.RandomState(seed)
    U, I = Rm.shape
    out = []
    for s in range(STEPS):
        rows, cols = rs.permutation(U)[:BLOCK[0]], rs.permutation(I)[:BLOCK[1]]
        if s == 0:
            rows[rows == 5] = rows[0]
            rows[0] = 5
            cols[cols == 0] = cols[3]
            cols[3] = 0
        assert len(set(rows)) == len(rows) and len(set(cols)) == len(cols)
        out.append((rows.astype(np.int64), cols.astype(np.int64)))
    return out


def run_case(ds, case, init, blocks, pair_seed, predict_users, cand):
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        rm.RecordingEvaluator.users = list(predict_users)
        model, sess, variables = build(ds, _hyper(case, 64), width, init)
        tabs, losses, pairs = [], [], []
        for s, (rows, cols) in enumerate(blocks):
            np.random.seed(pair_seed + s)
            p, n = model.pairwise_neg_sampling(rows, cols)
            assert len(p) > 0
            _, loss = sess.run([model.optimizer, model.cost], feed_dict=feed_of(model, rows, cols, p, n))
            losses.append(float(loss))
            pairs.append((np.asarray(p, np.int32), np.asarray(n, np.int32)))
            tabs.append([v.numpy() for v in variables])
        model.evaluate()
        full = _np(model.predict(list(predict_users), None), width)
        some = _np(model.predict(list(predict_users), [list(c) for c in cand]), width)
        out[tag] = dict(tabs=tabs, losses=losses, pairs=pairs, full=full, cand=some)
    for (pa, na), (pb, nb) in zip(out["f32"]["pairs"], out["f64"]["pairs"]):
        assert np.array_equal(pa, pb) and np.array_equal(na, nb)
    return out


def pack_tables(case, tabs_by_tag, init):
    out = {}
    for j, name in enumerate(R.NAMES):
        want = np.stack([t[j] for t in tabs_by_tag["f64"]]).astype(np.float64)
        twin = np.stack([t[j] for t in tabs_by_tag["f32"]]).astype(np.float64)
        out["%s_f64_%s" % (case, name)] = want - init[name].astype(np.float64)[None]
        out["%s_gap_%s" % (case, name)] = np.abs(twin - want).reshape(len(want), -1).max(axis=1, initial=0)
    return out


def run_epoch(ds, init, predict_users):
    """one whole train_model() of `default` at batch 48: the class draws its permutations and its negatives from
    numpy's stream; both widths see the same"""
    out = {}
    num_neg = R.CASES[R.EPOCH_CASE][4]
    for tag, width in WIDTHS:
        _reset_recorders()
        rm.RecordingEvaluator.users = list(predict_users)
        model, sess, variables = build(ds, _hyper(R.EPOCH_CASE, R.EPOCH_BATCH, H=R.EPOCH_H), width, init)
        fed, plain_run = [], sess.run

        def run(fetches, feed_dict=None, _fed=fed, _run=plain_run, _model=model):
            res = _run(fetches, feed_dict)
            if isinstance(fetches, list) and len(fetches) == 2:          # [optimizer, cost]: a training block
                _fed.append(dict(rows=np.asarray(feed_dict[_model.row_idx]).reshape(-1),
                                 cols=np.asarray(feed_dict[_model.col_idx]).reshape(-1),
                                 p=np.asarray(feed_dict[_model.input_P_cor]), n=np.asarray(feed_dict[_model.input_N_cor]),
                                 loss=float(res[1])))
            return res
        sess.run = run
        np.random.seed(EPOCH_SEED)
        model.train_model()
        line = [x for x in rm.MemoryLogger.lines if x.startswith("[iter 1 :")]
        assert len(line) == 1
        logged = float(re.match(r"\[iter 1 : loss : ([-0-9.eE+]+),", line[0]).group(1))
        out[tag] = dict(fed=fed, tabs=[[v.numpy() for v in variables]], logged=logged)
    a, b = out["f32"], out["f64"]
    assert len(a["fed"]) == len(b["fed"]) == 12
    for fa, fb in zip(a["fed"], b["fed"]):
        assert all(np.array_equal(fa[k], fb[k]) for k in ("rows", "cols", "p", "n"))
    Rm = ds.train_matrix
    for f in b["fed"]:
        # what the issue's seed search found must hold for THIS seed: a positive in every block, and every block row
        # with a positive keeps at least num_neg unobserved columns (else the reference raises)
        sub = Rm[f["rows"], :][:, f["cols"]].toarray()
        assert sub.sum() > 0 and len(f["p"]) == int(sub.sum()) * num_neg
        has = sub.sum(1) > 0
        assert np.all((sub.shape[1] - sub.sum(1))[has] >= max(num_neg, 17))
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_jca_ops()
    check_ops()
    Rm = toy_matrix(isolated=True)
    U, I = Rm.shape
    ds = rm.Dataset(Rm)
    out = dict(shape=np.asarray(Rm.shape, np.int64), indptr=Rm.indptr.astype(np.int64), indices=Rm.indices.astype(np.int32),
               cases=np.asarray(sorted(R.CASES)), steps=np.int64(STEPS), batch_epoch=np.int64(R.EPOCH_BATCH))
    rs = np.random.RandomState(7)
    predict_users = np.sort(rs.choice(U, N_PREDICT, replace=False)).astype(np.int32)
    cand = rs.randint(0, I, (N_PREDICT, 3)).astype(np.int32)
    out.update(predict_users=predict_users, predict_cand=cand)
    gaps = {}
    for k, case in enumerate(sorted(R.CASES)):
        H = R.CASES[case][5]
        init = R.init_tables(U, I, H, seed=1300 + k)
        blocks = make_blocks(Rm, case, 8100 + k)
        res = run_case(ds, case, init, blocks, 8200 + 10 * k, predict_users, cand)
        out["%s_init_seed" % case] = np.int64(1300 + k)
        out["%s_pair_seed" % case] = np.int64(8200 + 10 * k)
        for s, (rows, cols) in enumerate(blocks):
            out["%s_rows_%d" % (case, s)] = rows.astype(np.int32)
            out["%s_cols_%d" % (case, s)] = cols.astype(np.int32)
            out["%s_p_%d" % (case, s)], out["%s_n_%d" % (case, s)] = res["f64"]["pairs"][s]
        for tag, _ in WIDTHS:
            out["%s_loss_%s" % (case, tag)] = np.asarray(res[tag]["losses"], np.float64)
            out["predict_%s_%s" % (case, tag)] = res[tag]["full"]
            out["predict_%s_cand_%s" % (case, tag)] = res[tag]["cand"]
        out.update(pack_tables(case, {tag: res[tag]["tabs"] for tag, _ in WIDTHS}, init))
        gaps[case] = max(out["%s_gap_%s" % (case, n)].max(initial=0) for n in R.NAMES)
    init = R.init_tables(U, I, R.EPOCH_H, seed=1390)
    ep = run_epoch(ds, init, predict_users)
    for s, f in enumerate(ep["f64"]["fed"]):
        out["epoch_rows_%d" % s] = f["rows"].astype(np.int32)
        out["epoch_cols_%d" % s] = f["cols"].astype(np.int32)
        out["epoch_p_%d" % s] = f["p"].astype(np.int32)
        out["epoch_n_%d" % s] = f["n"].astype(np.int32)
    for tag, _ in WIDTHS:
        out["epoch_loss_%s" % tag] = np.asarray([f["loss"] for f in ep[tag]["fed"]], np.float64)
        out["epoch_logged_%s" % tag] = np.float64(ep[tag]["logged"])
    out.update(epoch_steps=np.int64(12), epoch_seed=np.int64(EPOCH_SEED), epoch_init_seed=np.int64(1390))
    out.update(pack_tables("epoch", {tag: ep[tag]["tabs"] for tag, _ in WIDTHS}, init))
    gaps["epoch"] = max(out["epoch_gap_%s" % n].max(initial=0) for n in R.NAMES)
    path = os.path.join(HERE, "tfgraph_jca.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); fp32 vs fp64 table gaps %s" % (
        path, os.path.getsize(path), {k: "%.3g" % v for k, v in gaps.items()}))


if __name__ == "__main__":
    main()
