"""Golden GRU4RecPlus trace produced by the REFERENCE's own GRU4RecPlus class
(model/sequential_recommender/GRU4RecPlus.py).

The class is loaded whole and unchanged with oracle/ref_models._load_file and runs under oracle/tf_shim.py, exactly as
make_golden_gru4rec.py does for GRU4Rec; the restated GRUCell, attach_ops and RecordingSession are that maker's.  Ops of
GRU4RecPlus.py the shim lacks beyond those (eye, reduce_max) are attached from here (attach_plus_ops), each checked on a
small hand-computed value; `multiply`, `exp`, `log`, `pow` and `reduce_sum(keep_dims=)` are the shim's own.

    python tests/golden/make_golden_gru4recplus.py              # needs the reference tree

Writes tests/golden/tfgraph_gru4recplus.npz, laid out as tfgraph_gru4rec.npz:
  indptr / indices / shape     the train pattern: toy_matrix(isolated=False) (157 x 131; items absent from training)
  seq_ptr / seq                every user's items by time: a seeded permutation of the row
  data_uit / offset_idx        as GRU4RecPlus._init_data builds them
  pop_cumsum                   as GRU4RecPlus.__init__ builds it (sample_alpha 0.75): one entry per item that OCCURS
  <case>_init_<var>            the initial variables of the case (float32), <var> of gru4rec_restatement.table_names
  <case>_X [steps, B] / _Y [steps, B + n_sample] / _reset [steps, B]
  <case>_rows_{E_in,Q,b}       the rows of that table that differ from their initial value at any step, in either width
  <case>_{f32,f64}_<var>       [steps, ...]: those rows (the cells' variables: whole) after each step MINUS their
                               initial value, in float64
  <case>_{f32,f64}_state<l>    [steps, B, n_l]: the fetched final_state of each step (before the reset)
  epoch_*                      one train_model() epoch at batch_size 16, n_sample 8 with a recording session:
                               epoch_perm, epoch_X [S, 16], epoch_Y [S, 24], epoch_zero [S, 16] (state rows all zero on
                               entry), the end tables as above under the case name `epoch`
  user_emb_{f32,f64}           _get_user_embeddings() after the last step of the case `bprmax_tanh_linear`
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
import make_golden_gru4rec as G               # noqa: E402
import gru4recplus_restatement as P           # noqa: E402

B_STEP, N_STEP, B_EPOCH, N_EPOCH, STEPS = 20, 12, 16, 8, 3
SAMPLE_ALPHA = 0.75
EPOCH_SEED = 4243


def load_gru4recplus():
    """the reference module model/sequential_recommender/GRU4RecPlus.py, executed under the shim"""
    saved_tf = tf_shim.install()
    saved = {k: sys.modules.get(k) for k in G._SHADOWED}
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
        sys.modules["data"] = types.ModuleType("data")
        ev = types.ModuleType("evaluator")
        ev.ProxyEvaluator = rm.RecordingEvaluator
        sys.modules["evaluator"] = ev
        model_pkg = types.ModuleType("model")
        model_pkg.__path__ = []
        sys.modules["model"] = model_pkg
        rm._load_file("model.AbstractRecommender", os.path.join(rm.REF, "model", "AbstractRecommender.py"))
        mod = rm._load_file("model.sequential_recommender.GRU4RecPlus",
                            os.path.join(rm.REF, "model", "sequential_recommender", "GRU4RecPlus.py"))
        sys.modules.pop("model.sequential_recommender.GRU4RecPlus", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


def attach_plus_ops():
    """make_golden_gru4rec.attach_ops, then the ops GRU4RecPlus.py needs beyond it, by their published definitions, each
    checked here on a small value"""
    import torch
    G.attach_ops()

    def eye(num_rows, num_columns=None, name=None, **_):
        cols = num_rows if num_columns is None else num_columns
        return tf_shim.Tensor(lambda r, c: torch.eye(int(r), int(c), dtype=tf_shim.float_dtype()), [num_rows, cols])

    def reduce_max(x, axis=None, keepdims=False, name=None, keep_dims=None):
        kd = bool(keepdims or keep_dims)
        return tf_shim.Tensor(lambda a: torch.max(a) if axis is None else torch.amax(a, dim=axis, keepdim=kd), [x])

    tf_shim.eye, tf_shim.reduce_max = eye, reduce_max
    run = lambda t: tf_shim._evaluate([t], {})[0]
    tf_shim.set_float("float64")
    x = tf_shim.constant(np.asarray([[1.0, -2.0, 3.0], [4.0, 5.0, -6.0]]))
    shp = tf_shim.shape(x)
    assert run(eye(shp[0], shp[1])).tolist() == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    assert run(eye(2)).tolist() == [[1.0, 0.0], [0.0, 1.0]]
    assert run(reduce_max(x, axis=1, keep_dims=True)).tolist() == [[3.0], [5.0]]
    assert run(reduce_max(x, axis=1)).tolist() == [3.0, 5.0]
    assert run(tf_shim.multiply(x, 1.0 - eye(shp[0], shp[1]))).tolist() == [[0.0, -2.0, 3.0], [4.0, 0.0, -6.0]]
    assert run(tf_shim.reduce_sum(x, axis=1, keep_dims=True)).tolist() == [[2.0], [3.0]]
    assert run(tf_shim.pow(x, 2)).tolist() == [[1.0, 4.0, 9.0], [16.0, 25.0, 36.0]]
    assert abs(float(run(tf_shim.log(tf_shim.exp(tf_shim.constant(np.asarray(1.5)))))) - 1.5) < 1e-15
    tf_shim.reset_default_graph()
    return True


def build(dataset, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    G.CELLS.clear()
    mod = load_gru4recplus()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "GRU4RecPlus"
    conf.update(hyper)
    sess = G.RecordingSession(seed=0)
    model = mod.GRU4RecPlus(sess, dataset, conf)
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess


def _variables(model):
    out = [model.input_embeddings, model.item_embeddings, model.item_biases]
    for cell in G.CELLS:
        out += list(cell.vars)
    return out


def make_batches(n_items, steps, B, n_sample, seed):
    """X and the positives hold duplicates, one item is an input and an output of the same step, the hub item 0 takes
    part on both sides; among the negatives: some row's positive, a duplicate pair and the hub item"""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        X, Y = rs.randint(1, n_items, B), rs.randint(1, n_items, B)
        X[1], Y[3], Y[4], X[6], Y[7] = X[0], Y[2], X[5], 0, 0
        assert len(set(X.tolist())) < B and len(set(Y.tolist())) < B and set(X.tolist()) & set(Y.tolist())
        if n_sample:
            neg = rs.randint(1, n_items, n_sample)
            neg[0], neg[2], neg[3] = Y[9], neg[1], 0
            assert neg[0] in Y and len(set(neg.tolist())) < n_sample
            Y = np.concatenate([Y, neg])
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
                state[l][list(G.RESETS.get(k, ()))] = 0
        out[tag] = (tabs, states)
        if with_predict is not None:
            users, cand = with_predict
            model.evaluate_model()
            out[tag + "_user_emb"] = _np(model.cur_user_embeddings, width)
            out[tag + "_predict"] = _np(model.predict(list(users), None), width)
            out[tag + "_predict_cand"] = _np(model.predict(list(users), [list(c) for c in cand]), width)
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
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["Y"], b["Y"]) and np.array_equal(a["zero"], b["zero"])
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_plus_ops()
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
               batch_epoch=np.int64(B_EPOCH), n_sample_epoch=np.int64(N_EPOCH), sample_alpha=np.float64(SAMPLE_ALPHA))
    lens = np.diff(ptr)
    order = np.argsort(-lens, kind="stable")
    predict_users = np.asarray([order[0], order[1], order[len(order) // 2], order[-1], 3], np.int32)
    cand = np.asarray([[3, 0, I - 1], [7, 7, 1], [0, 1, 2], [I - 1, I - 2, 5], [9, 8, 0]], np.int32)
    out.update(predict_users=predict_users, predict_cand=cand)
    gaps = {}
    for k, case in enumerate(sorted(P.CASES)):
        loss, hact, fact, layers, reg, bpr_reg, n_sample = P.CASES[case]
        assert n_sample in (0, N_STEP)
        hyper = dict(lr=P.LR, reg=reg, bpr_reg=bpr_reg, layers=list(layers), batch_size=B_STEP, loss=loss,
                     hidden_act=hact, final_act=fact, n_sample=n_sample, sample_alpha=SAMPLE_ALPHA, epochs=1, topk=20)
        names = P.table_names(len(layers))
        tables = P.init_tables(I, layers, seed=800 + k)
        init = [tables[n] for n in names]
        batches = make_batches(I, STEPS, B_STEP, n_sample, seed=600 + k)
        last = case == P.PREDICT_CASE
        res = run_case(ds, init, hyper, batches, (predict_users, cand) if last else None)
        for n, t in zip(names, init):
            out["%s_init_%s" % (case, n)] = t
        out[case + "_X"] = np.stack([b[0] for b in batches])
        out[case + "_Y"] = np.stack([b[1] for b in batches])
        reset = np.zeros((STEPS, B_STEP), bool)
        for s, slots in G.RESETS.items():
            reset[s, list(slots)] = True
        out[case + "_reset"] = reset
        out.update(G.pack_tables(case, names, {tag: res[tag][0] for tag, _ in WIDTHS}, init))
        for tag, _ in WIDTHS:
            for l in range(len(layers)):
                out["%s_%s_state%d" % (case, tag, l)] = np.stack([st[l] for st in res[tag][1]]).astype(np.float64)
        if last:
            for tag, _ in WIDTHS:
                out["user_emb_" + tag] = res[tag + "_user_emb"]
                out["predict_" + tag] = res[tag + "_predict"]
                out["predict_cand_" + tag] = res[tag + "_predict_cand"]
        gaps[case] = max(np.abs(out["%s_f32_%s" % (case, t)] - out["%s_f64_%s" % (case, t)]).max() for t in names)
    # _init_data and pop_cumsum as the class builds them, and one whole epoch
    loss, hact, fact, layers, reg, bpr_reg, _ = P.CASES[P.PREDICT_CASE]
    hyper = dict(lr=P.LR, reg=reg, bpr_reg=bpr_reg, layers=list(layers), batch_size=B_EPOCH, loss=loss, hidden_act=hact,
                 final_act=fact, n_sample=N_EPOCH, sample_alpha=SAMPLE_ALPHA, epochs=1, topk=20)
    model, _ = build(ds, hyper, "float64")
    out["data_uit"], out["offset_idx"] = model.data_uit.astype(np.int32), model.offset_idx.astype(np.int32)
    out["pop_cumsum"] = np.asarray(model.pop_cumsum, np.float64)
    assert len(out["pop_cumsum"]) < I                       # items absent from training (this matrix: the two highest ids)
    names = P.table_names(len(layers))
    tables = P.init_tables(I, layers, seed=890)
    init = [tables[n] for n in names]
    ep = run_epoch(ds, init, hyper)
    for n, t in zip(names, init):
        out["epoch_init_%s" % n] = t
    out.update(epoch_perm=ep["f64"]["perm"].astype(np.int64), epoch_X=ep["f64"]["X"], epoch_Y=ep["f64"]["Y"],
               epoch_zero=ep["f64"]["zero"], epoch_seed=np.int64(EPOCH_SEED))
    out.update(G.pack_tables("epoch", names, {tag: ep[tag]["tabs"] for tag, _ in WIDTHS}, init))
    gaps["epoch"] = max(np.abs(out["epoch_f32_%s" % t] - out["epoch_f64_%s" % t]).max() for t in names)
    path = os.path.join(HERE, "tfgraph_gru4recplus.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); %d epoch steps; %d of %d items occur; fp32 vs fp64 table gaps %s; user_emb gap %.3g; "
          "predict gap %.3g" % (path, os.path.getsize(path), len(out["epoch_X"]), len(out["pop_cumsum"]), I,
                                {k: "%.3g" % v for k, v in gaps.items()},
                                np.abs(out["user_emb_f32"] - out["user_emb_f64"]).max(),
                                np.abs(out["predict_f32"] - out["predict_f64"]).max()))


if __name__ == "__main__":
    main()
