"""Golden FPMC trace produced by the REFERENCE's own FPMC class (model/sequential_recommender/FPMC.py).

The class is loaded whole and unchanged with oracle/ref_models._load_file and runs under oracle/tf_shim.py, as
make_golden_fism.py does for FISM.  oracle/ref_models.load only knows model/general_recommender/, so this file
registers the same stand-ins itself (`util` re-exporting the reference's tool / learner functions, `data` with replay
samplers under the four names FPMC.py imports, `evaluator`, `model`) and loads the file from
model/sequential_recommender/.  The maker drives `sess.run((model.loss, model.optimizer), feed_dict)` itself;
train_model() is not called.  predict() is the reference's.

    python tests/golden/make_golden_fpmc.py              # needs the reference tree

Writes tests/golden/tfgraph_fpmc.npz:
  indptr / indices / shape     the train pattern: toy_matrix() (157 x 131)
  seq_ptr / seq                every user's items by time: a seeded permutation of the row
  UI_0 / IU_0 / IL_0 / LI_0    the initial tables (0.1 randn); hyper-parameters as scalars
  <case>_users/_recent/_items/_third   the batches [steps, B] (third = labels, or the negatives in the pairwise case)
  <case>_rows_{UI,IU,IL,LI}    the rows of that table that differ from its initial value at any step, in either width —
                               every other row equals its initial value after every step
  <case>_{f32,f64}_{UI,IU,IL,LI}   [steps, len(rows), d]: those rows after each step MINUS their initial value, in
                               float64; <case>_{f32,f64}_loss [steps]: the fetched (pre-update) loss
  predict_users, predict_{f32,f64}, predict_cand, predict_cand_{f32,f64}
                               predict() rows after the last step of the case `ce_adam`, full and candidate mode
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
import fpmc_restatement as P                  # noqa: E402

HYPER = dict(epochs=1, batch_size=64, embedding_size=16, reg_mf=0.01, learning_rate=0.01, learner="adam",
             is_pairwise=False, num_neg=4, loss_function="cross_entropy", init_method="normal", stddev=0.01, verbose=1,
             topk=20)
# case -> (hyper overrides, steps)
CASES = {
    "ce_adam": (dict(), 3),
    "square_adam": (dict(loss_function="square"), 3),
    "square_gd": (dict(loss_function="square", learner="gd"), 2),
    "square_adagrad": (dict(loss_function="square", learner="adagrad"), 2),
    "square_rmsprop": (dict(loss_function="square", learner="rmsprop"), 2),
    "square_momentum": (dict(loss_function="square", learner="momentum"), 2),
    "bpr_adam": (dict(loss_function="bpr", is_pairwise=True), 3),
}
B_POINT, B_PAIR = 60, 40

_SHADOWED = ("util", "util.tool", "util.learner", "data", "evaluator", "model", "model.AbstractRecommender",
             "model.sequential_recommender")


def load_fpmc():
    """the reference module model/sequential_recommender/FPMC.py, executed under the shim (ref_models.load's steps
    with the sequential family's imports)"""
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
        data = types.ModuleType("data")
        data.PairwiseSampler = data.PointwiseSampler = rm.ReplaySampler
        data.TimeOrderPointwiseSampler = data.TimeOrderPairwiseSampler = rm.ReplaySampler
        sys.modules["data"] = data
        ev = types.ModuleType("evaluator")
        ev.ProxyEvaluator = rm.RecordingEvaluator
        sys.modules["evaluator"] = ev
        model_pkg = types.ModuleType("model")
        model_pkg.__path__ = []
        sys.modules["model"] = model_pkg
        rm._load_file("model.AbstractRecommender", os.path.join(rm.REF, "model", "AbstractRecommender.py"))
        mod = rm._load_file("model.sequential_recommender.FPMC",
                            os.path.join(rm.REF, "model", "sequential_recommender", "FPMC.py"))
        sys.modules.pop("model.sequential_recommender.FPMC", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


def attach_ops():
    """ops of FPMC.py the shim lacks (their published definitions); none today — the hook make_golden_fism.py has"""
    for name in ("multiply", "reduce_sum", "placeholder", "log_sigmoid", "square"):
        assert hasattr(tf_shim, name), name


class TimedDataset(rm.Dataset):
    """rm.Dataset with the timestamps a UIRT file gives: time_matrix[u, i] = 1 + the item's place in the sequence"""

    def __init__(self, train, seqs):
        rm.Dataset.__init__(self, train)
        rows, cols, vals = [], [], []
        for u, s in seqs.items():
            rows += [u] * len(s)
            cols += s
            vals += list(range(1, len(s) + 1))
        self.time_matrix = sp.csr_matrix((np.asarray(vals, np.float64), (rows, cols)), shape=train.shape)
        self.seqs = seqs

    def get_user_train_dict(self, by_time=False):
        return dict(self.seqs) if by_time else rm.Dataset.get_user_train_dict(self)


def build(dataset, hyper, width):
    """ref_models.build for the sequential class"""
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    mod = load_fpmc()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "FPMC"
    conf.update(hyper)
    sess = tf_shim.Session(seed=0)
    model = mod.FPMC(sess, dataset, conf)
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess


# ------------------------------------------------------------------ inputs
def time_orders(R, seed=77):
    rs = np.random.RandomState(seed)
    return {u: rs.permutation(R.indices[R.indptr[u]:R.indptr[u + 1]]).astype(int).tolist()
            for u in range(R.shape[0]) if R.indptr[u + 1] > R.indptr[u]}


def make_batches(seqs, n_items, steps, pairwise, seed):
    """[(users, recent, items, third)] per step, windows (seq[k], seq[k+1]) of the users' sequences; negatives and
    label-0 items outside the user's sequence; every batch holds the five duplicate patterns (checked)"""
    rs = np.random.RandomState(seed)
    windows = [(u, s[k], s[k + 1]) for u, s in seqs.items() for k in range(len(s) - 1)]
    long = [u for u, s in seqs.items() if len(s) >= 3]
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
        s0 = seqs[u0]
        pos = [(u0, s0[0], s0[1]), (u0, s0[1], s0[2])]          # a user twice; s0[1] target here, recent there
        n_pos = B if pairwise else B // 2
        for k in rs.choice(len(windows), n_pos - len(pos), replace=False):
            pos.append(windows[k])
        if pairwise:
            negs = [neg(u) for u, _, _ in pos]
            for k in range(1, len(pos)):                          # the first positive is some other pair's negative
                if pos[0][2] not in seqs[pos[k][0]]:
                    negs[k] = pos[0][2]
                    break
            users, recent, items = ([p[c] for p in pos] for c in range(3))
            third = np.asarray(negs, np.int32)
        else:
            inst = [(u, l, i, 1.0) for u, l, i in pos]
            for k, (u, l, _) in enumerate(pos):                   # one label-0 instance per window
                inst.append((u, l, neg(u, pos[0][2] if k > 0 else None), 0.0))
            order = rs.permutation(len(inst))
            inst = [inst[k] for k in order]
            users, recent, items = ([p[c] for p in inst] for c in range(3))
            third = np.asarray([p[3] for p in inst], np.float32)
        assert len(users) == B
        pat = P.edge_patterns(users, recent, items, third, pairwise)
        assert all(pat.values()), pat
        out.append(tuple(np.asarray(x, np.int32) for x in (users, recent, items)) + (third,))
    return out


# ------------------------------------------------------------------ the runs
def run_case(ds, init, hyper, batches, predict_users=None, cand=None):
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, hyper, width)
        for var, t in zip((model.embeddings_UI, model.embeddings_IU, model.embeddings_IL, model.embeddings_LI), init):
            var.load(t)
        tabs, losses = [], []
        for users, recent, items, third in batches:
            feed = {model.user_input: users, model.item_input: items, model.item_input_recent: recent}
            feed[model.item_input_neg if hyper["is_pairwise"] else model.labels] = third
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=feed)
            losses.append(float(loss))
            tabs.append(tuple(v.numpy() for v in (model.embeddings_UI, model.embeddings_IU, model.embeddings_IL,
                                                  model.embeddings_LI)))
        out[tag] = (tabs, np.asarray(losses, np.float64))
        if predict_users is not None:
            out[tag + "_predict"] = _np(model.predict(list(predict_users), None), width)
            out[tag + "_predict_cand"] = _np(model.predict(list(predict_users), [list(c) for c in cand]), width)
    return out


def pack(case, res, init, batches):
    """rows that moved, per table, and their DIFFERENCE from the initial table in float64 (make_golden_fism.pack)"""
    init64 = [t.astype(np.float64) for t in init]
    out = {case + "_" + name: np.stack([b[c] for b in batches])
           for c, name in enumerate(("users", "recent", "items", "third"))}
    for j, name in enumerate(P.TABLES):
        moved = np.zeros(len(init[j]), bool)
        for tag, _ in WIDTHS:
            for tabs in res[tag][0]:
                moved |= (tabs[j].astype(np.float64) != init64[j]).any(axis=1)
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
    rs = np.random.RandomState(4210)
    init = [(0.1 * rs.randn(n, d)).astype(np.float32) for n in (U, I, I, I)]
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
               UI_0=init[0], IU_0=init[1], IL_0=init[2], LI_0=init[3], predict_users=predict_users, predict_cand=cand,
               reg_mf=np.float64(HYPER["reg_mf"]), learning_rate=np.float64(HYPER["learning_rate"]),
               cases=np.asarray(sorted(CASES)))
    gaps = {}
    for k, (case, (over, steps)) in enumerate(sorted(CASES.items())):
        hyper = dict(HYPER, **over)
        batches = make_batches(seqs, I, steps, hyper["is_pairwise"], seed=300 + k)
        last = case == "ce_adam"
        res = run_case(ds, init, hyper, batches, predict_users if last else None, cand if last else None)
        out.update(pack(case, res, init, batches))
        if last:
            for tag, _ in WIDTHS:
                out["predict_" + tag] = res[tag + "_predict"]
                out["predict_cand_" + tag] = res[tag + "_predict_cand"]
        gaps[case] = max(np.abs(out["%s_f32_%s" % (case, t)] - out["%s_f64_%s" % (case, t)]).max() for t in P.TABLES)
    path = os.path.join(HERE, "tfgraph_fpmc.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); fp32 vs fp64 table gaps %s" % (path, os.path.getsize(path),
                                                              {k: "%.3g" % v for k, v in gaps.items()}))


if __name__ == "__main__":
    main()
