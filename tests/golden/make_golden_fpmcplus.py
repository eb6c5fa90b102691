"""Golden FPMCplus trace produced by the REFERENCE's own FPMCplus class (model/sequential_recommender/FPMCplus.py).

The class is loaded whole and unchanged with oracle/ref_models._load_file and runs under oracle/tf_shim.py with the
module stand-ins make_golden_fpmc.py registers for FPMC (make_golden_npe.load_npe's steps on the other file) and the
call forms make_golden_nais.attach_ops adds (`reshape`, `stack`, `tile`, `ones`).  The maker drives
`sess.run((model.loss, model.optimizer), feed_dict)` itself; train_model() is not called.  predict() is the reference's.

    python tests/golden/make_golden_fpmcplus.py              # needs the reference tree

Writes tests/golden/tfgraph_fpmcplus.npz (arrays and hyper-parameter values only):
  indptr / indices / shape     the train pattern: make_golden_fossil.train_matrix(3) (157 x 131)
  seq_ptr / seq                every user's items by time: a seeded permutation of the row
  UI_0 / IU_0 / IL_0 / LI_0 / W_0 / b_0      the initial tables (0.1 randn; W 0.2 randn [3d, w]; b [1, w])
  <case>_h_0                   the initial h [w, 1]: ones in the shipped configuration `bpr_adam`, seeded values near 1
                               in every other case, so that h's own gradient path shows
  <case>_users/_recents/_items/_third   the batches [steps, B] ([steps, B, L] recents; third = the negatives or the
                               labels); every batch holds a user twice, an item that is a target here and a recent
                               there, one instance with the same item twice among its recents and, in the pairwise
                               cases, a negative that is another instance's positive (asserted)
  <case>_rows_{UI,IU,IL,LI}    the rows of that table that differ from its initial value at any step, in either width
  <case>_{f32,f64}_{UI,IU,IL,LI}   [steps, len(rows), d]: those rows after each step MINUS their initial value, float64
  <case>_{f32,f64}_{W,b,h}     [steps, ...]: the dense tables whole, MINUS their initial value, float64
  <case>_{f32,f64}_loss [steps]    the fetched (pre-update) loss
  predict_users, predict_{f32,f64}, predict_cand, predict_cand_{f32,f64}
                               predict() rows after the last step of the case `bpr_adam` (L = 3), full and candidate
                               mode, for users with |R_u| >= L (the reference fails on the others)
No case at L = 1: the reference's rank-2 placeholder cannot take the sampler's 1-D recents there.
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
from make_golden_tfgraph import WIDTHS, _np, _reset_recorders   # noqa: E402
from make_golden_fpmc import TimedDataset, time_orders, _SHADOWED   # noqa: E402
from make_golden_fossil import train_matrix   # noqa: E402
import make_golden_nais as MN                 # noqa: E402
import fpmcplus_restatement as P              # noqa: E402

HYPER = dict(epochs=1, batch_size=64, embedding_size=16, weight_size=16, high_order=3, reg_mf=0.01, reg_w=0.02,
             learning_rate=0.01, learner="adam", is_pairwise=True, num_neg=4, loss_function="bpr",
             embed_init_method="normal", weight_init_method="normal", stddev=0.01, verbose=1, topk=20)
STEPS = {P.PREDICT_CASE: 3}                   # every other case: 2
B = 60
VARS = ("embeddings_UI", "embeddings_IU", "embeddings_IL", "embeddings_LI", "W", "b", "h")


def load_fpmcplus():
    """the reference module model/sequential_recommender/FPMCplus.py, executed under the shim (make_golden_npe.load_npe's
    steps, with both time-order samplers as the replay sampler)"""
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
        data.TimeOrderPointwiseSampler = data.TimeOrderPairwiseSampler = rm.ReplaySampler
        sys.modules["data"] = data
        ev = types.ModuleType("evaluator")
        ev.ProxyEvaluator = rm.RecordingEvaluator
        sys.modules["evaluator"] = ev
        model_pkg = types.ModuleType("model")
        model_pkg.__path__ = []
        sys.modules["model"] = model_pkg
        rm._load_file("model.AbstractRecommender", os.path.join(rm.REF, "model", "AbstractRecommender.py"))
        mod = rm._load_file("model.sequential_recommender.FPMCplus",
                            os.path.join(rm.REF, "model", "sequential_recommender", "FPMCplus.py"))
        sys.modules.pop("model.sequential_recommender.FPMCplus", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


def build(dataset, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    mod = load_fpmcplus()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "FPMCplus"
    conf.update(hyper)
    sess = tf_shim.Session(seed=0)
    model = mod.FPMCplus(sess, dataset, conf)
    assert {u: list(s) for u, s in model.train_dict.items()} == dataset.seqs      # csr_to_user_dict_bytime
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess


# ------------------------------------------------------------------ inputs
def make_batches(seqs, n_items, L, steps, pairwise, seed):
    """[(users, recents [B, L], items, third)] per step: windows of the users' sequences (recents oldest first, as the
    sampler delivers them).  Pairwise: B windows, negatives outside the user's sequence, one of them another
    instance's positive.  Pointwise: B / 2 windows with label 1 and one label-0 instance per window."""
    rs = np.random.RandomState(seed)
    win = lambda u, k: (u, seqs[u][k - L:k], seqs[u][k])
    windows = [win(u, j) for u, s in seqs.items() for j in range(L, len(s))]
    long = [u for u, s in seqs.items() if len(s) >= L + 3]
    assert long
    out = []
    for _ in range(steps):
        u0 = long[rs.randint(len(long))]
        u1, r1, i1 = win(u0, L + 1)
        # one user twice, seq[L] the target of its first window and a recent of its second; the second window once
        # more with its first recent replaced by its second (an item twice among the recents)
        pos = [win(u0, L), (u1, r1, i1), (u1, [r1[1]] + r1[1:], i1)]
        n_pos = B if pairwise else B // 2
        for j in rs.choice(len(windows), n_pos - len(pos), replace=False):
            pos.append(windows[j])

        def neg(u):
            while True:
                j = int(rs.randint(n_items))
                if j not in seqs[u]:
                    return j
        if pairwise:
            negs = [neg(u) for u, _, _ in pos]
            for k in range(1, len(pos)):                          # the first positive is some other pair's negative
                if pos[0][2] not in seqs[pos[k][0]]:
                    negs[k] = pos[0][2]
                    break
            inst = [(u, r, i, j) for (u, r, i), j in zip(pos, negs)]
        else:
            inst = [(u, r, i, 1.0) for u, r, i in pos] + [(u, r, neg(u), 0.0) for u, r, _ in pos]
        inst = [inst[j] for j in rs.permutation(len(inst))]
        users, recents, items = ([p[c] for p in inst] for c in range(3))
        third = np.asarray([p[3] for p in inst], np.int32 if pairwise else np.float32)
        assert len(users) == B
        pat = P.edge_patterns(users, recents, items, third, pairwise)
        assert all(pat.values()), pat
        out.append((np.asarray(users, np.int32), np.asarray(recents, np.int32).reshape(B, L),
                    np.asarray(items, np.int32), third))
    return out


# ------------------------------------------------------------------ the runs
def run_case(ds, init, hyper, batches, predict_users=None, cand=None):
    out = {}
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, hyper, width)
        variables = [getattr(model, v) for v in VARS]
        for var, t in zip(variables, init):
            var.load(t)
        tabs, losses = [], []
        for users, recents, items, third in batches:
            feed = {model.user_input: users, model.item_input: items, model.item_input_recent: recents}
            feed[model.item_input_neg if hyper["is_pairwise"] else model.labels] = third
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=feed)
            losses.append(float(loss))
            tabs.append(tuple(v.numpy() for v in variables))
        out[tag] = (tabs, np.asarray(losses, np.float64))
        if predict_users is not None:
            out[tag + "_predict"] = _np(model.predict(list(predict_users), None), width)
            out[tag + "_predict_cand"] = _np(model.predict(list(predict_users), [list(c) for c in cand]), width)
    return out


def pack(case, res, init, batches):
    """make_golden_npe.pack for the four row tables (the moved rows, their DIFFERENCE from the initial table in
    float64); the dense tables whole, as differences as well"""
    init64 = [t.astype(np.float64) for t in init]
    out = {case + "_" + name: np.stack([b[c] for b in batches])
           for c, name in enumerate(("users", "recents", "items", "third"))}
    for j, name in enumerate(P.TABLES):
        if name in P.ROWS:
            moved = np.zeros(len(init[j]), bool)
            for tag, _ in WIDTHS:
                for tabs in res[tag][0]:
                    moved |= (tabs[j].astype(np.float64) != init64[j]).any(axis=1)
            rows = np.flatnonzero(moved).astype(np.int32)
            out["%s_rows_%s" % (case, name)] = rows
        else:
            rows = slice(None)
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
    MN.attach_ops()
    R = train_matrix(3)
    U, I = R.shape
    seqs = time_orders(R)
    ds = TimedDataset(R, seqs)
    d, w = HYPER["embedding_size"], HYPER["weight_size"]
    rs = np.random.RandomState(4223)
    init = [(0.1 * rs.randn(n, d)).astype(np.float32) for n in (U, I, I, I)]
    init += [(0.2 * rs.randn(3 * d, w)).astype(np.float32), (0.1 * rs.randn(1, w)).astype(np.float32)]
    longer = [u for u, s in seqs.items() if len(s) >= 3]
    predict_users = np.asarray(longer[:4], np.int32)
    cand = np.asarray([[3, 0, I - 1], [7, 7, 1], [0, 1, 2], [I - 1, I - 2, 5]], np.int32)
    ptr = np.zeros(U + 1, np.int64)
    for u, s in seqs.items():
        ptr[u + 1] = len(s)
    ptr = np.cumsum(ptr)
    out = dict(indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32), shape=np.asarray(R.shape, np.int64),
               seq_ptr=ptr, seq=np.asarray([i for u in sorted(seqs) for i in seqs[u]], np.int32),
               UI_0=init[0], IU_0=init[1], IL_0=init[2], LI_0=init[3], W_0=init[4], b_0=init[5],
               predict_users=predict_users, predict_cand=cand,
               reg_mf=np.float64(HYPER["reg_mf"]), reg_w=np.float64(HYPER["reg_w"]),
               learning_rate=np.float64(HYPER["learning_rate"]), cases=np.asarray(sorted(P.CASES)))
    gaps = {}
    for k, (case, (loss, learner, pairwise, L)) in enumerate(sorted(P.CASES.items())):
        hyper = dict(HYPER, loss_function=loss, learner=learner, is_pairwise=pairwise, high_order=L)
        batches = make_batches(seqs, I, L, STEPS.get(case, 2), pairwise, seed=900 + k)
        last = case == P.PREDICT_CASE
        h0 = np.ones((w, 1), np.float32) if last else (1.0 + 0.1 * rs.randn(w, 1)).astype(np.float32)
        out[case + "_h_0"] = h0
        res = run_case(ds, init + [h0], hyper, batches, predict_users if last else None, cand if last else None)
        out.update(pack(case, res, init + [h0], batches))
        if last:
            assert all(len(seqs[int(u)]) >= L for u in predict_users)
            for tag, _ in WIDTHS:
                out["predict_" + tag] = res[tag + "_predict"]
                out["predict_cand_" + tag] = res[tag + "_predict_cand"]
        gaps[case] = {t: "%.3g" % np.abs(out["%s_f32_%s" % (case, t)] - out["%s_f64_%s" % (case, t)]).max()
                      for t in P.TABLES}
    assert any(not np.all(out[c + "_h_0"] == 1) for c in P.CASES)
    path = os.path.join(HERE, "tfgraph_fpmcplus.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); fp32 vs fp64 gaps per table:" % (path, os.path.getsize(path)))
    for case in sorted(gaps):
        print("  %-16s %s" % (case, gaps[case]))


if __name__ == "__main__":
    main()
