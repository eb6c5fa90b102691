"""Golden Fossil trace produced by the REFERENCE's own Fossil class (model/sequential_recommender/Fossil.py).

The class is loaded whole and unchanged with oracle/ref_models._load_file and runs under oracle/tf_shim.py, as
make_golden_fpmc.py does for FPMC.  Fossil calls `tf.constant(value, dtype, shape)` (attached as make_golden_fism.py
does) and `tf.tile` / `tf.stack` (as make_golden_nais.py does).  The maker drives
`sess.run((model.loss, model.optimizer), feed_dict)` itself on feeds built to the structure the reference's generators
state (positive / label 1: the history without the item, num_idx = |R_u| - 1; negative / label 0: the whole history,
num_idx = |R_u|; recents seq[idx-1], ..., seq[idx-L], most recent first); train_model() and the generators are not
called (they alias one list per user and mutate it).  predict() is the reference's.

    python tests/golden/make_golden_fossil.py              # needs the reference tree

Writes tests/golden/tfgraph_fossil.npz:
  indptr / indices / shape     the train pattern: toy_matrix() (157 x 131), rows trimmed so that users with 2, 3 and 4
                               items exist (|R_u| < L, = L, = L + 1 at L = 3)
  seq_ptr / seq                every user's items by time: a seeded permutation of the row
  c1_0 / Q_0 / bias_0 / eta_0 [U, 3] / eta_bias_0 [3]
                               the initial tables; a case at high_order L starts from the first L columns of eta
  <case>_users/_recents/_items/_third   the batches [steps, B] ([steps, B, L] recents, most recent first; third =
                               labels, or the negatives in the pairwise cases)
  <case>_rows_<table>          the rows of that table that differ from its initial value at any step, in either width
  <case>_{f32,f64}_<table>     those rows after each step MINUS their initial value, in float64;
  <case>_{f32,f64}_loss [steps]   the fetched (pre-update) loss
  predict_users, predict_{f32,f64}, predict_cand, predict_cand_{f32,f64}
                               predict() rows after the last step of the case `bpr_adagrad`, full and candidate mode,
                               for users with |R_u| > L + 1, = L + 1 and = L (none with |R_u| < L: the reference's feed
                               is ragged there)
"""
import os
import sys
import types

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_models as rm          # noqa: E402
from oracle import tf_shim                    # noqa: E402
from make_golden_tfgraph import WIDTHS, _np, _reset_recorders, toy_matrix   # noqa: E402
import make_golden_fism as MF                 # noqa: E402
import make_golden_nais as MN                 # noqa: E402
from make_golden_fpmc import TimedDataset, time_orders   # noqa: E402
import fossil_restatement as P                # noqa: E402

HYPER = dict(epochs=1, batch_size=64, embedding_size=16, regs=[0.0, 0.0, 0.0], alpha=0.5, learning_rate=0.01,
             learner="adagrad", is_pairwise=True, high_order=3, num_neg=4, loss_function="bpr", init_method="uniform",
             stddev=0.01, verbose=1, topk=20)
STEPS = {"bpr_adagrad": 3}
B_POINT, B_PAIR = 48, 32

_SHADOWED = ("util", "util.tool", "util.learner", "util.data_generator", "util.data_iterator", "data", "evaluator",
             "model", "model.AbstractRecommender", "model.sequential_recommender")


def load_fossil():
    """the reference module model/sequential_recommender/Fossil.py, executed under the shim"""
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
        # train_model() alone uses these two: stand-ins that import
        util.data_generator = types.ModuleType("util.data_generator")
        it = types.ModuleType("util.data_iterator")
        it.DataIterator = type("DataIterator", (), {})
        sys.modules["util"], sys.modules["util.data_generator"], sys.modules["util.data_iterator"] = \
            util, util.data_generator, it
        ev = types.ModuleType("evaluator")
        ev.ProxyEvaluator = rm.RecordingEvaluator
        sys.modules["evaluator"] = ev
        model_pkg = types.ModuleType("model")
        model_pkg.__path__ = []
        sys.modules["model"] = model_pkg
        rm._load_file("model.AbstractRecommender", os.path.join(rm.REF, "model", "AbstractRecommender.py"))
        mod = rm._load_file("model.sequential_recommender.Fossil",
                            os.path.join(rm.REF, "model", "sequential_recommender", "Fossil.py"))
        sys.modules.pop("model.sequential_recommender.Fossil", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


def attach_ops():
    """tf.constant with a positional shape (make_golden_fism.py), tf.tile and tf.stack (make_golden_nais.py)"""
    MN.attach_ops()


def build(dataset, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    mod = load_fossil()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "Fossil"
    conf.update(hyper)
    sess = tf_shim.Session(seed=0)
    model = mod.Fossil(sess, dataset, conf)
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess


# ------------------------------------------------------------------ inputs
def train_matrix(L=3):
    """toy_matrix() with the rows of three users trimmed to L - 1, L and L + 1 items where it lacks such a user"""
    R = toy_matrix().tolil()
    deg = np.asarray([len(r) for r in R.rows])
    long = [u for u in np.argsort(-deg, kind="stable")]
    for want in (L - 1, L, L + 1):
        if not (deg == want).any():
            u = long.pop()
            while deg[u] <= L + 1:
                u = long.pop()
            R.rows[u], R.data[u] = R.rows[u][:want], R.data[u][:want]
            deg[u] = want
    R = R.tocsr()
    R.sort_indices()
    return R


def make_batches(seqs, n_items, L, steps, pairwise, seed):
    """[(users, recents [B, L], items, third)] per step: windows of the users' sequences, recents most recent first;
    negatives and label-0 items outside the user's sequence; every batch holds the duplicate patterns (checked)"""
    rs = np.random.RandomState(seed)
    win = lambda u, k: (u, seqs[u][k - L:k][::-1], seqs[u][k])
    windows = [win(u, k) for u, s in seqs.items() for k in range(L, len(s))]
    long = [u for u, s in seqs.items() if len(s) >= L + 3]
    short = [u for u, s in seqs.items() if len(s) == L + 1]
    B = B_PAIR if pairwise else B_POINT

    def neg(u, prefer=None):
        if prefer is not None and prefer not in seqs[u]:
            return prefer
        while True:
            j = int(rs.randint(n_items))
            if j not in seqs[u]:
                return j

    out = []
    for _ in range(steps):
        u0 = long[rs.randint(len(long))]
        # one user three times: seq[L] is the target of the first window, eta column 0 of the second, column 1 of the
        # third; and a user with a single window
        pos = [win(u0, L), win(u0, L + 1), win(u0, L + 2), win(short[0], L)]
        n_pos = B if pairwise else B // 2
        for k in rs.choice(len(windows), n_pos - len(pos), replace=False):
            pos.append(windows[k])
        if pairwise:
            negs = [neg(u) for u, _, _ in pos]
            for k in range(1, len(pos)):                          # the first positive is some other pair's negative
                if pos[0][2] not in seqs[pos[k][0]]:
                    negs[k] = pos[0][2]
                    break
            users, recents, items = ([p[c] for p in pos] for c in range(3))
            third = np.asarray(negs, np.int32)
        else:
            inst = [(u, r, i, 1.0) for u, r, i in pos]
            for k, (u, r, _) in enumerate(pos):                   # one label-0 instance per window
                inst.append((u, r, neg(u, pos[0][2] if k > 0 else None), 0.0))
            inst = [inst[k] for k in rs.permutation(len(inst))]
            users, recents, items = ([p[c] for p in inst] for c in range(3))
            third = np.asarray([p[3] for p in inst], np.float32)
        assert len(users) == B
        pat = P.edge_patterns(users, recents, items, third, pairwise)
        assert all(pat.values()), pat
        out.append((np.asarray(users, np.int32), np.asarray(recents, np.int32).reshape(B, L),
                    np.asarray(items, np.int32), third))
    return out


def feed_of(R, users, items, positive):
    """histories / num_idx as the generators state them: positive: the row without the item, |R_u| - 1; else the
    whole row, |R_u|"""
    hist, num = [], []
    for u, i, y in zip(users, items, positive):
        its = R.indices[R.indptr[u]:R.indptr[u + 1]].tolist()
        if y:
            its.remove(int(i))
        num.append(len(its))
        hist.append(its)
    return hist, np.asarray(num, np.float32)


# ------------------------------------------------------------------ the runs
def _vars(model):
    return (model.c1, model.embedding_Q, model.bias, model.eta, model.eta_bias)


def run_case(ds, R, init, hyper, batches, predict_users=None, cand=None):
    out, I = {}, R.shape[1]
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, hyper, width)
        for var, t in zip(_vars(model), init):
            var.load(t.reshape(1, -1) if var is model.eta_bias else t)
        tabs, losses = [], []
        for users, recents, items, third in batches:
            feed = {model.user_input_id: users, model.item_input: items, model.item_input_recent: recents}
            if hyper["is_pairwise"]:
                hp, np_ = feed_of(R, users, items, [1] * len(users))
                hn, nn = feed_of(R, users, third, [0] * len(users))
                feed.update({model.user_input: MF.pad(hp, I), model.user_input_neg: MF.pad(hn, I), model.num_idx: np_,
                             model.num_idx_neg: nn, model.item_input_neg: third})
            else:
                h, n = feed_of(R, users, items, third > 0.5)
                feed.update({model.user_input: MF.pad(h, I), model.num_idx: n, model.labels: third})
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=feed)
            losses.append(float(loss))
            tabs.append(tuple(v.numpy().reshape(-1) if v is model.eta_bias else v.numpy() for v in _vars(model)))
        out[tag] = (tabs, np.asarray(losses, np.float64))
        if predict_users is not None:
            out[tag + "_predict"] = _np(np.stack(model.predict(list(predict_users), None)), width)
            out[tag + "_predict_cand"] = _np(np.stack(model.predict(list(predict_users), [list(c) for c in cand])),
                                             width)
    return out


def pack(case, res, init, batches):
    """rows that moved, per table, and their DIFFERENCE from the initial table in float64 (make_golden_fpmc.pack)"""
    init64 = [t.astype(np.float64) for t in init]
    out = {case + "_" + name: np.stack([b[c] for b in batches])
           for c, name in enumerate(("users", "recents", "items", "third"))}
    for j, name in enumerate(P.TABLES):
        moved = np.zeros(len(init[j]), bool)
        for tag, _ in WIDTHS:
            for tabs in res[tag][0]:
                diff = tabs[j].astype(np.float64) != init64[j]
                moved |= diff.any(axis=1) if diff.ndim == 2 else diff
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
    R = train_matrix()
    U, I = R.shape
    deg = np.diff(R.indptr)
    assert all((deg == n).any() for n in (1, 2, 3, 4)) and (deg == 0).any(), np.bincount(deg)[:6]
    seqs = time_orders(R)
    ds = TimedDataset(R, seqs)
    d = HYPER["embedding_size"]
    rs = np.random.RandomState(4211)
    c1, Q = ((0.1 * rs.randn(I, d)).astype(np.float32) for _ in range(2))
    bias = (0.1 * rs.randn(I)).astype(np.float32)
    eta, eta_bias = (0.3 * rs.randn(U, 3)).astype(np.float32), (0.3 * rs.randn(3)).astype(np.float32)
    by_len = lambda f: [u for u, s in seqs.items() if f(len(s))]
    predict_users = np.asarray(by_len(lambda n: n > 4)[:3] + by_len(lambda n: n == 4)[:1] + by_len(lambda n: n == 3)[:1],
                               np.int32)
    cand = np.asarray([[3, 0, I - 1], [7, 7, 1], [0, 1, 2], [I - 1, I - 2, 5], [9, 8, 0]], np.int32)
    ptr = np.zeros(U + 1, np.int64)
    for u, s in seqs.items():
        ptr[u + 1] = len(s)
    ptr = np.cumsum(ptr)
    out = dict(indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32), shape=np.asarray(R.shape, np.int64),
               seq_ptr=ptr, seq=np.asarray([i for u in sorted(seqs) for i in seqs[u]], np.int32),
               c1_0=c1, Q_0=Q, bias_0=bias, eta_0=eta, eta_bias_0=eta_bias, predict_users=predict_users,
               predict_cand=cand, learning_rate=np.float64(HYPER["learning_rate"]), cases=np.asarray(sorted(P.CASES)))
    gaps = {}
    for k, (case, (loss, learner, pairwise, L, regs, alpha)) in enumerate(sorted(P.CASES.items())):
        hyper = dict(HYPER, loss_function=loss, learner=learner, is_pairwise=pairwise, high_order=L, regs=list(regs),
                     alpha=alpha)
        batches = make_batches(seqs, I, L, STEPS.get(case, 2), pairwise, seed=500 + k)
        init = [c1, Q, bias, np.ascontiguousarray(eta[:, :L]), eta_bias[:L].copy()]
        last = case == "bpr_adagrad"
        res = run_case(ds, R, init, hyper, batches, predict_users if last else None, cand if last else None)
        out.update(pack(case, res, init, batches))
        if last:
            for tag, _ in WIDTHS:
                out["predict_" + tag] = res[tag + "_predict"]
                out["predict_cand_" + tag] = res[tag + "_predict_cand"]
        gaps[case] = max(np.abs(out["%s_f32_%s" % (case, t)] - out["%s_f64_%s" % (case, t)]).max(initial=0)
                         for t in P.TABLES)
    path = os.path.join(HERE, "tfgraph_fossil.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); fp32 vs fp64 table gaps %s" % (path, os.path.getsize(path),
                                                              {k: "%.3g" % v for k, v in gaps.items()}))


if __name__ == "__main__":
    main()
