"""Golden CDAE trace produced by the REFERENCE's own class (model/general_recommender/CDAE.py).

The class is loaded whole and unchanged (make_golden_neumf.load_class) and run under oracle/tf_shim.py.  The ops it
needs beyond the shim's are attached here by their published definitions [EXT: tensorflow r1.12] and put on a small
hand-computed value first (check_ops): sparse_placeholder (with the sparse_retain / `* scalar` /
sparse_tensor_dense_matmul forms of a FED sparse tensor, and random_uniform over a fed shape), unique,
squared_difference, gather, reshape, zeros_initializer.  Nothing under oracle/ changes.  `util.tool` (dropout_sparse,
l2_loss, inner_product, randint_choice) and `util.data_iterator` are the reference's own files.

    python tests/golden/make_golden_cdae.py              # needs the reference tree

The stand-in gives `en_embeddings` ApplyAdam (it is read by a matmul) and the sparse form to `user_embedding`,
`de_embeddings` and `item_bias`; both forms sweep every row.

Writes tests/golden/tfgraph_cdae.npz:
  shape, indptr, indices       the toy matrix (157 x 131)
  <case>_init_seed             the initial variables are cdae_restatement.init_tables(157, 131, d, seed)
  <case>_users [S, 6]          the fed users; slot 2 repeats slot 0, slot 1 holds as a NEGATIVE the first train item of
                               slot 0, and where the case has dropout every entry of slot 3 is dropped
  <case>_neg_<s>, _negptr_<s>  the np.unique'd negatives of step s, flat, and their offsets per slot
  <case>_unif_<s>              the uniforms behind the mask of step s, one per input entry (kept: floor(u + keep) == 1)
  <case>_loss_{f32,f64} [S]    the loss of each step (before its update)
  <case>_f64_<var> [S, ...]    the variable after each step of the float64 run MINUS its initial value
  <case>_gap_<var> [S]         max |float32 run - float64 run| of the variable after each step
  predict_users, predict_cand, predict_<case>_unif, predict_<case>_{f32,f64}
                               predict() after the last step for 27 users, [27, 131] (candidate mode returns the same
                               rows in the reference: the candidates are predict_cand's columns of them)
  epoch_*                      one train_model() epoch of `default` at batch_size 16 through the recording session under
                               numpy seed epoch_seed: per step s the fed users, items, labels, remap_idx and sparse
                               indices as the class built them, the negatives and uniforms; the end tables under the
                               case name `epoch`
"""
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
import make_golden_neumf as N                 # noqa: E402
import cdae_restatement as R                  # noqa: E402

B_STEP, B_EPOCH, STEPS = 6, 16, 3
EPOCH_SEED = 7411
N_PREDICT = 27
VARS = R.TABLES                               # the class creates its variables in this order


# ------------------------------------------------------------------ the ops the shim lacks
class FedSparse:
    """tf.sparse_placeholder: a sparse tensor whose indices [nnz, 2], values [nnz] and row count are fed"""

    def __init__(self, indices, values, n_rows, name=None):
        self.indices, self.values, self.n_rows, self.name = indices, values, n_rows, name

    def __mul__(self, o):                     # SparseTensor.__mul__ scales the values
        return FedSparse(self.indices, tf_shim.multiply(self.values, o), self.n_rows)
    __rmul__ = __mul__


def attach_cdae_ops():
    import torch
    T = tf_shim.Tensor

    def sparse_placeholder(dtype, shape=None, name=None):
        return FedSparse(tf_shim.placeholder(tf_shim.int64, [None, 2], name="%s/indices" % name),
                         tf_shim.placeholder(dtype, [None], name="%s/values" % name),
                         tf_shim.placeholder(tf_shim.int32, [], name="%s/rows" % name), name)

    shim_retain, shim_spmm, shim_uniform = tf_shim.sparse_retain, tf_shim.sparse_tensor_dense_matmul, \
        tf_shim.random_uniform
    if getattr(shim_retain, "cdae", False):
        return

    def sparse_retain(sp_input, to_retain, name=None):
        """sparse_ops.sparse_retain keeps the entries whose flag is True; a dropped entry stays as an exact 0"""
        if not isinstance(sp_input, FedSparse):
            return shim_retain(sp_input, to_retain, name)
        return FedSparse(sp_input.indices, T(lambda v, m: v * m.to(v.dtype), [sp_input.values, to_retain]),
                         sp_input.n_rows)
    sparse_retain.cdae = True

    def sparse_tensor_dense_matmul(sp_a, b, name=None, **kw):
        """out[r] = sum over the stored entries of row r, in the order stored, of value * b[col]"""
        if not isinstance(sp_a, FedSparse):
            return shim_spmm(sp_a, b, name, **kw)

        def f(idx, v, n, x):
            out = torch.zeros(int(n), x.shape[1], dtype=x.dtype)
            return out.index_add(0, idx[:, 0], v.detach().unsqueeze(1) * x.index_select(0, idx[:, 1]))
        return T(f, [sp_a.indices, sp_a.values, sp_a.n_rows, b])

    def random_uniform(shape, *a, **k):
        """a shape list that holds a fed scalar ([nnz] in dropout_sparse)"""
        if isinstance(shape, (list, tuple)) and any(isinstance(s, T) for s in shape):
            shape = T(lambda *xs: torch.tensor([int(x) for x in xs]), list(shape))
        return shim_uniform(shape, *a, **k)

    def unique(x, out_idx=None, name=None):
        """array_ops.unique: the distinct values in order of first occurrence, and every element's index among them"""
        def first(a):
            seen, vals = set(), []
            for v in a.reshape(-1).tolist():
                if v not in seen:
                    seen.add(v)
                    vals.append(v)
            return torch.tensor(vals, dtype=torch.int64)
        y = T(first, [x])
        return y, T(lambda a, u: torch.tensor([u.tolist().index(v) for v in a.reshape(-1).tolist()], dtype=torch.int64),
                    [x, y])

    def squared_difference(x, y, name=None):
        return T(lambda a, b: (a - b) * (a - b), [x, y])

    def gather(params, indices, name=None, **_):
        return tf_shim.nn.embedding_lookup(params, indices)      # kind "gather": IndexedSlices for a variable

    def reshape(tensor, shape, name=None):
        return T(lambda a: a.reshape(*[int(s) for s in shape]), [tensor])

    def zeros_initializer(dtype=None):
        return lambda shape, dtype=None, partition_info=None: np.zeros(tuple(int(s) for s in shape), np.float32)

    for fn in (sparse_placeholder, sparse_retain, sparse_tensor_dense_matmul, random_uniform, unique,
               squared_difference, gather, reshape, zeros_initializer):
        setattr(tf_shim, fn.__name__, fn)


class CdaeSession(tf_shim.Session):
    """the shim's Session with a fed sparse tensor taken apart, and a log of the feeds"""

    def __init__(self, *a, **k):
        tf_shim.Session.__init__(self, *a, **k)
        self.feed_log = None

    def run(self, fetches, feed_dict=None):
        fd = {}
        for k, v in (feed_dict or {}).items():
            if isinstance(k, FedSparse):
                idx, val, shp = v
                fd[k.indices] = np.asarray(idx, np.int64).reshape(-1, 2)
                fd[k.values] = np.asarray(val)
                fd[k.n_rows] = int(shp[0])
            else:
                fd[k] = v
        if self.feed_log is not None and feed_dict is not None:
            self.feed_log.append({k.name: np.array(v) for k, v in fd.items()})
        return tf_shim.Session.run(self, fetches, fd)


def check_ops():
    """every attached op on a small hand-computed value"""
    tf = tf_shim
    tf.set_float("float64")
    tf.reset_default_graph()
    sess = CdaeSession(seed=0)
    y, idx = tf.unique(tf.constant(np.asarray([4, 2, 4, 7, 2])))
    assert sess.run(y).tolist() == [4, 2, 7] and sess.run(idx).tolist() == [0, 1, 0, 2, 1]
    a, b = tf.constant(np.asarray([1.0, 5.0])), tf.constant(np.asarray([3.0, 4.5]))
    assert sess.run(tf.squared_difference(a, b)).tolist() == [4.0, 0.25]
    v = tf.Variable(np.asarray([5.0, 6.0, 7.0]))
    g = tf.gather(v, tf.constant(np.asarray([2, 0, 2])))
    assert g.kind == "gather" and sess.run(g).tolist() == [7.0, 5.0, 7.0]
    assert sess.run(tf.reshape(v, shape=[1, -1])).tolist() == [[5.0, 6.0, 7.0]]
    z = tf.zeros_initializer()([2, 3])
    assert z.shape == (2, 3) and not z.any()
    # a fed 3 x 4 sparse matrix, entries (0,1) (0,3) (2,0); keep flags from uniforms 0.7, 0.2, 0.5 at keep 0.5;
    # scaled by 2: rows [2 W1, 0, 2 W0]
    sp = tf.sparse_placeholder(tf.float32, [None, 4], name="sp")
    n = tf.placeholder(tf.int32, name="n")
    W = tf.Variable(np.asarray([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]]))
    mask = tf.cast(tf.floor(tf.random_uniform([n]) + 0.5), dtype=tf.bool)
    out = tf.sparse_tensor_dense_matmul(tf.sparse_retain(sp, mask) * 2.0, W)
    sess.inject([np.asarray([0.7, 0.2, 0.5], np.float32)])
    got = sess.run(out, feed_dict={sp: (np.asarray([[0, 1], [0, 3], [2, 0]]), np.ones(3, np.float32), (3, 4)), n: 3})
    assert got.tolist() == [[6.0, 8.0], [0.0, 0.0], [2.0, 4.0]], got
    tf.reset_default_graph()
    return True


# ------------------------------------------------------------------ the class
class Dataset(rm.Dataset):
    def to_csr_matrix(self):
        return self.train_matrix.copy()


def build(ds, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    tf_shim._GRAPH.collections = {}
    mod = N.load_class("CDAE")
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "CDAE"
    conf.update(hyper)
    sess = CdaeSession(seed=0)
    model = mod.CDAE(sess, ds, conf)
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    variables = list(tf_shim._GRAPH.variables)
    U, I = ds.train_matrix.shape
    d = hyper["hidden_dim"]
    assert [tuple(v.value.shape) for v in variables] == [(U, d), (I, d), (d,), (I, d), (I,)]
    return model, sess, variables


def _hyper(case, batch):
    act, loss, reg, dropout, d = R.CASES[case]
    return dict(lr=R.LR, reg=reg, hidden_dim=d, dropout=dropout, num_neg=R.NUM_NEG, epochs=1, batch_size=batch,
                hidden_act=act, loss_func=loss)


def feed_of(model, batch, n_items):
    """the feed the class builds in train_model (CDAE.py:126-140), from a restated batch"""
    ptr = batch["entry_ptr"]
    rows = np.repeat(np.arange(len(batch["users"])), np.diff(ptr))
    indices = np.stack([rows, batch["in_items"]], axis=1)
    return {model.users_ph: batch["users"].astype(np.int32), model.remap_idx_ph: batch["slot"].astype(np.int32),
            model.items_ph: batch["items"].astype(np.int32),
            model.sp_mat_ph: (indices, np.ones(len(rows), np.float32), (len(batch["users"]), n_items)),
            model.labels_ph: batch["labels"].astype(np.float32), model.dropout_ph: 0.0,
            model.noise_shape_ph: int(len(rows))}


def make_batches(Rm, steps, seed, dropout):
    """per step (users, negatives, uniforms): slot 2 repeats slot 0's user; slot 1 has slot 0's first train item among
    its negatives; with dropout, every entry of slot 3 is dropped (uniform 0)"""
    rs = np.random.RandomState(seed)
    U, I = Rm.shape
    deg = np.diff(Rm.indptr)
    pool = np.flatnonzero((deg >= 1) & (deg <= 12))
    out = []
    for _ in range(steps):
        while True:
            users = rs.choice(pool, B_STEP, replace=False)
            shared = int(Rm.indices[Rm.indptr[users[0]]])
            row1 = Rm.indices[Rm.indptr[users[1]]:Rm.indptr[users[1] + 1]]
            if shared not in row1:
                break
        users[2] = users[0]
        negs = []
        for s, u in enumerate(users):
            row = Rm.indices[Rm.indptr[u]:Rm.indptr[u + 1]]
            allowed = np.setdiff1d(np.arange(I), row)
            drawn = rs.choice(allowed, len(row) * R.NUM_NEG, replace=True)
            if s == 1:
                drawn = np.r_[drawn, shared]
            negs.append(np.unique(drawn).astype(np.int32))
        b = R.build_batch(Rm.indptr, Rm.indices, users, negs)
        unif = (rs.randint(0, 1 << 20, len(b["items"])) / float(1 << 20)).astype(np.float32)
        if dropout > 0:
            unif[b["entry_ptr"][3]:b["entry_ptr"][4]] = 0.0
        out.append((users.astype(np.int32), negs, unif, b))
    return out


def run_case(ds, case, init, batches, predict=None):
    I = ds.train_matrix.shape[1]
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess, variables = build(ds, _hyper(case, B_STEP), width)
        for var, n in zip(variables, VARS):
            var.load(init[n])
        tabs, losses = [], []
        for users, negs, unif, b in batches:
            sess.inject([unif])
            loss, _ = sess.run((model.train_opt.loss, model.train_opt), feed_dict=feed_of(model, b, I))
            losses.append(float(loss))
            tabs.append([v.numpy() for v in variables])
        out[tag] = (tabs, losses)
        if predict is not None:
            users, unif = predict
            sess.inject([unif])
            out[tag + "_predict"] = _np(model.predict(list(users), None), width)
    return out


def pack_tables(case, tabs_by_tag, init):
    out = {}
    for j, name in enumerate(VARS):
        want = np.stack([t[j] for t in tabs_by_tag["f64"]]).astype(np.float64)
        twin = np.stack([t[j] for t in tabs_by_tag["f32"]]).astype(np.float64)
        out["%s_f64_%s" % (case, name)] = want - init[name].astype(np.float64)[None]
        out["%s_gap_%s" % (case, name)] = np.abs(twin - want).reshape(len(want), -1).max(axis=1, initial=0)
    return out


def run_epoch(ds, init):
    """one whole train_model() of `default` at batch 16: the class draws its own negatives (numpy's stream) and the
    session the uniforms; both widths are fed the same"""
    keep = np.float32(1.0) - np.float32(R.CASES[R.EPOCH_CASE][3])
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        rm.RecordingEvaluator.users = [0]
        model, sess, variables = build(ds, _hyper(R.EPOCH_CASE, B_EPOCH), width)
        for var, n in zip(variables, VARS):
            var.load(init[n])
        np.random.seed(EPOCH_SEED)
        sess.feed_log, sess.draw_log = [], []
        model.train_model()
        fed = [f for f in sess.feed_log if "items" in f]           # predict() feeds no items
        unif = [a for kind, a in sess.draw_log if kind == "random_uniform"][:len(fed)]
        assert all(len(u) == len(f["sp_mat/indices"]) for u, f in zip(unif, fed))
        out[tag] = dict(fed=fed, unif=unif, tabs=[[v.numpy() for v in variables]])
    a, b = out["f32"], out["f64"]
    assert len(a["fed"]) == len(b["fed"])
    for fa, fb, ua, ub in zip(a["fed"], b["fed"], a["unif"], b["unif"]):
        assert all(np.array_equal(fa[k], fb[k]) for k in fa) and np.array_equal(ua, ub)
        assert np.array_equal(np.floor(ua + keep), np.floor(ua.astype(np.float64) + float(keep)))
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_cdae_ops()
    check_ops()
    Rm = toy_matrix(isolated=True)
    U, I = Rm.shape
    ds = Dataset(Rm)
    out = dict(shape=np.asarray(Rm.shape, np.int64), indptr=Rm.indptr.astype(np.int64), indices=Rm.indices.astype(np.int32),
               lr=np.float64(R.LR), num_neg=np.int64(R.NUM_NEG), cases=np.asarray(sorted(R.CASES)),
               batch_step=np.int64(B_STEP), batch_epoch=np.int64(B_EPOCH), steps=np.int64(STEPS))
    rs = np.random.RandomState(7)
    predict_users = np.sort(rs.choice(U, N_PREDICT, replace=False)).astype(np.int32)
    cand = rs.randint(0, I, (N_PREDICT, 3)).astype(np.int32)
    n_pred = int(sum(Rm.indptr[u + 1] - Rm.indptr[u] for u in predict_users))
    out.update(predict_users=predict_users, predict_cand=cand)
    gaps = {}
    for k, case in enumerate(sorted(R.CASES)):
        act, loss, reg, dropout, d = R.CASES[case]
        init = R.init_tables(U, I, d, seed=900 + k)
        batches = make_batches(Rm, STEPS, 7500 + k, dropout)
        punif = (rs.randint(0, 1 << 20, n_pred) / float(1 << 20)).astype(np.float32)
        res = run_case(ds, case, init, batches, (predict_users, punif))
        out["%s_init_seed" % case] = np.int64(900 + k)
        out["%s_users" % case] = np.stack([b[0] for b in batches])
        for s, (users, negs, unif, b) in enumerate(batches):
            out["%s_neg_%d" % (case, s)] = np.concatenate(negs).astype(np.int32)
            out["%s_negptr_%d" % (case, s)] = np.concatenate([[0], np.cumsum([len(n) for n in negs])]).astype(np.int64)
            out["%s_unif_%d" % (case, s)] = unif
        for tag, _ in WIDTHS:
            out["%s_loss_%s" % (case, tag)] = np.asarray(res[tag][1], np.float64)
            out["predict_%s_%s" % (case, tag)] = res[tag + "_predict"]
        out["predict_%s_unif" % case] = punif
        out.update(pack_tables(case, {tag: res[tag][0] for tag, _ in WIDTHS}, init))
        gaps[case] = max(out["%s_gap_%s" % (case, n)].max(initial=0) for n in VARS)
    d = R.CASES[R.EPOCH_CASE][4]
    init = R.init_tables(U, I, d, seed=990)
    ep = run_epoch(ds, init)
    fed, unif = ep["f64"]["fed"], ep["f64"]["unif"]
    for s, (f, u) in enumerate(zip(fed, unif)):
        out["epoch_users_%d" % s] = f["user"].astype(np.int32)
        out["epoch_items_%d" % s] = f["items"].astype(np.int32)
        out["epoch_labels_%d" % s] = f["labels"].astype(np.float32)
        out["epoch_idx_%d" % s] = f["remap_idx"].astype(np.int32)
        out["epoch_spidx_%d" % s] = f["sp_mat/indices"].astype(np.int32)
        out["epoch_unif_%d" % s] = u.astype(np.float32)
    out.update(epoch_steps=np.int64(len(fed)), epoch_seed=np.int64(EPOCH_SEED), epoch_init_seed=np.int64(990))
    out.update(pack_tables("epoch", {tag: ep[tag]["tabs"] for tag, _ in WIDTHS}, init))
    gaps["epoch"] = max(out["epoch_gap_%s" % n].max(initial=0) for n in VARS)
    path = os.path.join(HERE, "tfgraph_cdae.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); %d epoch steps; fp32 vs fp64 table gaps %s" % (
        path, os.path.getsize(path), len(fed), {k: "%.3g" % v for k, v in gaps.items()}))


if __name__ == "__main__":
    main()
