"""Golden FISM trace produced by the REFERENCE's own FISM class (model/general_recommender/FISM.py).

The class is imported whole and unchanged through oracle/ref_models.py and runs under oracle/tf_shim.py, as
make_golden_wrmf.py does for WRMF.  FISM calls `tf.constant(value, dtype, shape)` and `tf.zeros(<int>)`, two call
forms the shim does not carry: this file attaches them before the class is loaded (their published definitions: a
tensor of `shape` filled with `value`; a vector of zeros).  `util.data_generator` (the reference's file, executed
where it lies) and a stand-in `util.data_iterator` are registered in sys.modules so that the class imports.

The maker drives `sess.run((model.loss, model.optimizer), feed_dict)` itself on padded feeds it builds by the rule of
util/data_generator.py:29-54 (positive: the history without the item, num_idx = |R_u|; negative: the whole history,
num_idx = |R_u| + 1); train_model() is not called (its generator draws from numpy's global stream, and its pairwise
generator hands the graph empty histories — the pairwise case here feeds the structure the pointwise generator
states).  predict() is the reference's.

    python tests/golden/make_golden_fism.py              # needs /root/reference

Writes tests/golden/tfgraph_fism.npz:
  indptr / indices / shape     the train pattern: toy_matrix() (157 x 131) on a widened item set, plus appended users
                               with 64, 65 and 1,100 items (histories of 63 / 64 / 65 items, and one longer than any
                               chunk a kernel may pick)
  c1_0 / Q0 / bias_0           the initial tables (the bias away from zero, see main()); hyper-parameters as scalars
  <case>_users/_items/_third   the batches [steps, B] (third = labels, or the negatives in the pairwise case)
  <case>_rows_{c1,Q,bias}      the rows of that table that differ from its initial value at any step, in either width —
                               every other row equals its initial value after every step
  <case>_{f32,f64}_{c1,Q}      [steps, len(rows), d] and <case>_{f32,f64}_bias [steps, len(rows)]: those rows after
                               each step MINUS their initial value, in float64 (value = initial + difference: exact
                               for f32, within 1e-15 for f64); <case>_{f32,f64}_loss [steps]: the fetched (pre-update) loss
  predict_users, predict_{f32,f64}, predict0_{f32,f64}
                               predict() rows after the last step of the case `square_adam`, and of untrained tables
                               with alpha = 0
  struct_*                     what the reference's _get_pointwise_all_likefism_data yields on the toy matrix, per
                               instance: user, item, label, num_idx, history length, excluded item or -1
"""
import os
import sys
import types

import numpy as np
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_models as rm          # noqa: E402
from oracle import tf_shim                    # noqa: E402
from make_golden_tfgraph import WIDTHS, _np, _reset_recorders, toy_matrix   # noqa: E402

N_ITEMS = 1200
HYPER = dict(batch_size=64, epochs=1, embedding_size=16, regs=[0.01, 0.02], alpha=0.5, num_neg=4, learning_rate=0.01,
             learner="adam", topk=20, loss_function="square", is_pairwise=False, init_method="normal", stddev=0.01,
             verbose=1)
# case -> (hyper overrides, steps, steps in which the 1,100-item user takes part)
CASES = {
    "square_adam": (dict(), 3, (2,)),
    "ce_adam": (dict(loss_function="cross_entropy"), 3, ()),
    "square_gd": (dict(learner="gd"), 2, ()),
    "square_adagrad": (dict(learner="adagrad"), 2, ()),
    "square_rmsprop": (dict(learner="rmsprop"), 2, ()),
    "square_momentum": (dict(learner="momentum"), 2, ()),
    "bpr_adam": (dict(loss_function="bpr", is_pairwise=True), 3, (2,)),
}


# ------------------------------------------------------------------ the two call forms FISM needs on top of the shim
def _constant(value, dtype=None, shape=None, name=None, **_):
    if shape is None:
        return tf_shim._Const(value)
    return tf_shim._Const(torch.full([int(s) for s in shape], float(value), dtype=tf_shim.float_dtype()))


def _zeros(shape, dtype=None, name=None, **_):
    shape = [int(shape)] if isinstance(shape, (int, np.integer)) else [int(s) for s in shape]
    return tf_shim.Tensor(lambda: torch.zeros(*shape, dtype=tf_shim.float_dtype()), [])


def attach_ops():
    tf_shim.constant = _constant
    tf_shim.zeros = _zeros


def register_util_modules():
    """util.data_generator: the reference's file; util.data_iterator: FISM.py imports DataIterator, train_model()
    alone uses it"""
    saved_tf = tf_shim.install()
    saved = {k: sys.modules.get(k) for k in ("util", "util.tool")}
    try:
        util = types.ModuleType("util")
        util.__path__ = []
        sys.modules["util"] = util
        rm._load_file("util.tool", os.path.join(rm.REF, "util", "tool.py"))
        gen = rm._load_file("util.data_generator", os.path.join(rm.REF, "util", "data_generator.py"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)
    it = types.ModuleType("util.data_iterator")
    it.DataIterator = type("DataIterator", (), {})
    sys.modules["util.data_iterator"] = it
    return gen


# ------------------------------------------------------------------ inputs
def train_matrix():
    toy = toy_matrix().tocoo()
    U = toy.shape[0]
    rows, cols = toy.row.tolist(), toy.col.tolist()
    rs = np.random.RandomState(64)
    for k, deg in enumerate((64, 65)):
        rows += [U + k] * deg
        cols += np.sort(rs.choice(N_ITEMS - 40, deg, replace=False)).tolist()
    rows += [U + 2] * 1100
    cols += (np.arange(1100) + 50).tolist()
    R = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(U + 3, N_ITEMS))
    R.sum_duplicates()
    R.data[:] = 1.0
    R.sort_indices()
    return R


def make_batches(R, steps, big_steps, pairwise, seed):
    """[(users, items, third)] per step: a user twice, an item twice, positives whose excluded item is the first / the
    last of the row, an empty history (pointwise), histories of 1, 63, 64, 65 items"""
    rs = np.random.RandomState(seed)
    U = R.shape[0] - 3
    u64, u65, big = U, U + 1, U + 2
    deg = np.diff(R.indptr)
    row = lambda u: R.indices[R.indptr[u]:R.indptr[u + 1]]
    one = [u for u in range(U) if deg[u] == 1]
    two = [u for u in range(U) if deg[u] == 2]
    has0 = [u for u in range(U) if deg[u] > 2 and row(u)[0] == 0]
    no0 = [u for u in range(U) if deg[u] > 2 and row(u)[0] != 0]
    assert one and two and has0 and no0

    def neg(u):
        while True:
            j = int(rs.randint(R.shape[1]))
            if j not in set(row(u).tolist()):
                return j

    out = []
    for k in range(steps):
        inst = []                                             # (user, item, positive?)
        inst += [(u64, int(row(u64)[0]), 1), (u64, int(row(u64)[-1]), 1), (u64, neg(u64), 0)]     # |H| = 63, 63, 64
        inst += [(u65, neg(u65), 0), (u65, int(row(u65)[7]), 1)]                                  # |H| = 65, 64
        a, b = has0[k % len(has0)], no0[k % len(no0)]
        inst += [(a, 0, 1), (b, 0, 0)]                                                            # item 0 twice
        t = two[k % len(two)]
        inst += [(t, int(row(t)[1]), 1)]                                                          # |H| = 1
        if not pairwise:
            o = one[k % len(one)]
            inst += [(o, int(row(o)[0]), 1), (o, neg(o), 0)]                                      # |H| = 0 and 1
        if k in big_steps:
            inst += [(big, int(row(big)[0]), 1), (big, neg(big), 0)]
        for u in rs.choice([u for u in range(U) if deg[u] > 2], 12 if k in big_steps else 13, replace=False):
            its = row(int(u))
            inst += [(int(u), int(its[rs.randint(len(its))]), 1), (int(u), neg(int(u)), 0)]
        if pairwise:                                          # a pair per positive: (u, i, sampled j)
            pos = [(u, i) for u, i, y in inst if y == 1]
            users, items = [u for u, _ in pos], [i for _, i in pos]
            third = np.asarray([neg(u) for u in users], np.int32)
            assert 2 * len(users) <= 64
        else:
            order = rs.permutation(len(inst))
            inst = [inst[j] for j in order]
            users, items = [u for u, _, _ in inst], [i for _, i, _ in inst]
            third = np.asarray([float(y) for _, _, y in inst], np.float32)
            assert len(users) <= 64
        out.append((np.asarray(users, np.int32), np.asarray(items, np.int32), third))
    return out


def feed_of(R, users, items, positive):
    """histories / num_idx of util/data_generator.py:29-54 for instances (user, item, positive?)"""
    hist, num = [], []
    for u, i, y in zip(users, items, positive):
        its = R.indices[R.indptr[u]:R.indptr[u + 1]].tolist()
        if y:
            its.remove(int(i))
            num.append(len(its) + 1)
        else:
            num.append(len(its) + 1)
        hist.append(its)
    return hist, np.asarray(num, np.float32)


def pad(hist, value):
    L = max(1, max(len(h) for h in hist))
    out = np.full((len(hist), L), value, np.int32)
    for k, h in enumerate(hist):
        out[k, :len(h)] = h
    return out


# ------------------------------------------------------------------ the runs
def run_case(R, c1_0, Q0, bias_0, hyper, batches, predict_users=None):
    out, I = {}, R.shape[1]
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess, _ = rm.build("FISM", rm.Dataset(R), hyper, width)
        model.c1.load(c1_0)
        model.embedding_Q.load(Q0)
        model.bias.load(bias_0)
        tabs, losses = [], []
        for users, items, third in batches:
            if hyper["is_pairwise"]:
                hp, np_ = feed_of(R, users, items, [1] * len(users))
                hn, nn = feed_of(R, users, third, [0] * len(users))
                feed = {model.user_input: pad(hp, I), model.user_input_neg: pad(hn, I), model.num_idx: np_,
                        model.num_idx_neg: nn, model.item_input: items, model.item_input_neg: third}
            else:
                h, n = feed_of(R, users, items, third > 0.5)
                feed = {model.user_input: pad(h, I), model.num_idx: n, model.item_input: items, model.labels: third}
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=feed)
            losses.append(float(loss))
            tabs.append((model.c1.numpy(), model.embedding_Q.numpy(), model.bias.numpy()))
        out[tag] = (tabs, np.asarray(losses, np.float64))
        if predict_users is not None:
            out[tag + "_predict"] = _np(np.stack(model.predict(list(predict_users), None)), width)
    return out


def pack(case, res, c1_0, Q0, bias_0, batches):
    """rows that moved, per table, and their DIFFERENCE from the initial table in float64 (the value is initial + difference: exact for f32,
    within an ulp for f64) — unmoved entries are zeros and cost nothing"""
    init = (c1_0.astype(np.float64), Q0.astype(np.float64), bias_0.astype(np.float64))
    B = max(len(b[0]) for b in batches)
    assert all(len(b[0]) == B for b in batches)
    out = {case + "_users": np.stack([b[0] for b in batches]), case + "_items": np.stack([b[1] for b in batches]),
           case + "_third": np.stack([b[2] for b in batches])}
    for j, name in enumerate(("c1", "Q", "bias")):
        moved = np.zeros(len(Q0), bool)
        for tag, _ in WIDTHS:
            for tabs in res[tag][0]:
                moved |= (tabs[j].astype(np.float64) != init[j]).reshape(len(Q0), -1).any(axis=1)
        rows = np.flatnonzero(moved).astype(np.int32)
        out["%s_rows_%s" % (case, name)] = rows
        for tag, width in WIDTHS:
            delta = np.stack([t[j].astype(np.float64)[rows] - init[j][rows] for t in res[tag][0]])
            back = (init[j][rows][None] + delta).astype(np.float32 if width == "float32" else np.float64)
            want = np.stack([t[j][rows] for t in res[tag][0]])
            assert np.array_equal(back, want) if width == "float32" else np.abs(back - want).max(initial=0) < 1e-15
            out["%s_%s_%s" % (case, tag, name)] = delta
    for tag, _ in WIDTHS:
        out["%s_%s_loss" % (case, tag)] = res[tag][1]
    return out


def structure_fixture(gen):
    """the reference's pointwise generator on the toy matrix (users with a train row: it raises KeyError on the rest)"""
    toy = toy_matrix()
    keep = np.flatnonzero(np.diff(toy.indptr) > 0)
    R = toy[keep]
    ds = rm.Dataset(R)
    np.random.seed(7)
    hist, num, items, labels = gen._get_pointwise_all_likefism_data(ds, 4, ds.get_user_train_dict())
    users, excl = [], []
    it = iter(range(len(hist)))
    for u in range(R.shape[0]):
        row = R.indices[R.indptr[u]:R.indptr[u + 1]].tolist()
        for _ in range(len(row) * 5):
            k = next(it)
            users.append(u)
            missing = sorted(set(row) - set(hist[k]))
            assert set(hist[k]) <= set(row) and len(missing) <= 1
            excl.append(missing[0] if missing else -1)
    i32 = lambda x: np.asarray(x, np.int32)
    return dict(struct_indptr=R.indptr.astype(np.int64), struct_indices=R.indices.astype(np.int32),
                struct_shape=np.asarray(R.shape, np.int64), struct_user=i32(users), struct_item=i32(items),
                struct_label=i32(labels), struct_num_idx=i32(num), struct_hist_len=i32([len(h) for h in hist]),
                struct_excluded=i32(excl))


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_ops()
    gen = register_util_modules()
    R = train_matrix()
    U, I = R.shape
    d = HYPER["embedding_size"]
    rs = np.random.RandomState(1307)
    c1_0 = (0.1 * rs.randn(I, d)).astype(np.float32)
    Q0 = (0.1 * rs.randn(I, d)).astype(np.float32)
    # a bias away from zero: with bias = 0 an empty history scores exactly 0, the one point where the derivative of
    # the stand-in's sigmoid cross-entropy (torch's |x|' = 0 at 0) is not TF's (0.5 - label)
    bias_0 = (0.01 * rs.randn(I)).astype(np.float32)
    one = int(np.flatnonzero(np.diff(R.indptr) == 1)[0])
    hubby = int(np.argmax(np.diff(R.indptr)[:U - 3]))
    some = [int(u) for u in np.flatnonzero(np.diff(R.indptr)[:U - 3] > 2) if u not in (one, hubby)][3::40][:3]
    predict_users = np.asarray([one, hubby] + some + [U - 3, U - 2, U - 1], np.int32)
    out = dict(indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32), shape=np.asarray(R.shape, np.int64),
               c1_0=c1_0, Q0=Q0, bias_0=bias_0, predict_users=predict_users, alpha=np.float64(HYPER["alpha"]),
               regs=np.asarray(HYPER["regs"], np.float64), learning_rate=np.float64(HYPER["learning_rate"]),
               cases=np.asarray(sorted(CASES)))
    gaps = {}
    for k, (case, (over, steps, big_steps)) in enumerate(sorted(CASES.items())):
        hyper = dict(HYPER, **over)
        batches = make_batches(R, steps, big_steps, hyper["is_pairwise"], seed=100 + k)
        res = run_case(R, c1_0, Q0, bias_0, hyper, batches, predict_users if case == "square_adam" else None)
        out.update(pack(case, res, c1_0, Q0, bias_0, batches))
        if case == "square_adam":
            out["predict_f32"], out["predict_f64"] = res["f32_predict"], res["f64_predict"]
        gaps[case] = max(np.abs(out["%s_f32_%s" % (case, t)] - out["%s_f64_%s" % (case, t)]).max() for t in ("c1", "Q"))
    res0 = run_case(R, c1_0, Q0, bias_0, dict(HYPER, alpha=0.0), [], predict_users)
    out["predict0_f32"], out["predict0_f64"] = res0["f32_predict"], res0["f64_predict"]
    out.update(structure_fixture(gen))
    path = os.path.join(HERE, "tfgraph_fism.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); fp32 vs fp64 table gaps %s" % (path, os.path.getsize(path),
                                                              {k: "%.3g" % v for k, v in gaps.items()}))


if __name__ == "__main__":
    main()
