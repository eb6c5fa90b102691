"""Golden NPE trace produced by the REFERENCE's own NPE class (model/sequential_recommender/NPE.py).

The class is loaded whole and unchanged with oracle/ref_models._load_file and runs under oracle/tf_shim.py (which has
tf.nn.relu: its gradient passes where the input is strictly positive, TF's ReluGrad — checked in attach_ops), with the
module stand-ins make_golden_fpmc.py registers for FPMC.  The maker drives
`sess.run((model.loss, model.optimizer), feed_dict)` itself; train_model() is not called.  predict() is the
reference's.

    python tests/golden/make_golden_npe.py              # needs the reference tree

Writes tests/golden/tfgraph_npe.npz:
  indptr / indices / shape     the train pattern: make_golden_fossil.train_matrix(3) (157 x 131; users with 1, 2, 3 and
                               4 items exist)
  seq_ptr / seq                every user's items by time: a seeded permutation of the row
  P_0 / V_0 / W_0              the initial tables (0.1 randn) with PLANTED ZEROS: for each of three reserved windows
                               (user u, recents r0..r4, target i = the user's sixth item) column 0 of P[u] is 0, column 1
                               of V[i] is 0, and column 2 of W holds 0.125, -0.125, 0, 0.25, -0.25 in r0..r4: the context
                               sum of the last 5, the last 3 and the last 2 cancels to exactly 0 while its members are
                               not 0; dyadic values, so float32 and float64 cancel alike
  zero_users / zero_recents / zero_items   the reserved windows [3] / [3, 5] / [3]; window k is held out of every batch
                               before step k, in every role, so that its rows still hold their initial values when
                               step k looks them up; a case at high_order L uses the last L recents
  <case>_users/_recents/_items/_labels   the batches [steps, B] ([steps, B, L] recents, oldest first); every batch
                               holds a user twice, an item that is a target here and a recent there, and one window
                               with the same item twice among its recents (its first recent replaced by its second)
  <case>_rows_{P,V,W}          the rows of that table that differ from its initial value at any step, in either width
  <case>_{f32,f64}_{P,V,W}     [steps, len(rows), d]: those rows after each step MINUS their initial value, in float64;
  <case>_{f32,f64}_loss [steps]   the fetched (pre-update) loss
  predict_users, predict_{f32,f64}, predict_cand, predict_cand_{f32,f64}
                               predict() rows after the last step of the case `ce_adam` (L = 3), full and candidate
                               mode: users with |R_u| >= 3, with |R_u| = 2 (sliced to 1) and |R_u| = 1
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
import npe_restatement as P                   # noqa: E402

HYPER = dict(epochs=1, batch_size=64, embedding_size=16, reg=0.01, learning_rate=0.01, learner="adam", high_order=3,
             num_neg=4, loss_function="cross_entropy", init_method="normal", stddev=0.01, verbose=1, topk=20)
STEPS = {P.PREDICT_CASE: 3}                   # every other case: 2
B = 60
W_MAX = 5                                     # recents per reserved window: the longest high_order among the cases
VARS = ("embeddings_UI", "embeddings_IU", "embeddings_IL")          # P, V, W


def load_npe():
    """the reference module model/sequential_recommender/NPE.py, executed under the shim (make_golden_fpmc.load_fpmc's
    steps)"""
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
        data.TimeOrderPointwiseSampler = rm.ReplaySampler
        sys.modules["data"] = data
        ev = types.ModuleType("evaluator")
        ev.ProxyEvaluator = rm.RecordingEvaluator
        sys.modules["evaluator"] = ev
        model_pkg = types.ModuleType("model")
        model_pkg.__path__ = []
        sys.modules["model"] = model_pkg
        rm._load_file("model.AbstractRecommender", os.path.join(rm.REF, "model", "AbstractRecommender.py"))
        mod = rm._load_file("model.sequential_recommender.NPE",
                            os.path.join(rm.REF, "model", "sequential_recommender", "NPE.py"))
        sys.modules.pop("model.sequential_recommender.NPE", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


def attach_ops():
    """nothing to add: the shim has every op of NPE.py.  Its relu's gradient is checked here on the values the
    planted zeros rest on: 0 and -0 pass nothing, as TF's ReluGrad (features > 0)."""
    import torch
    for name in ("multiply", "reduce_sum", "placeholder"):
        assert hasattr(tf_shim, name), name
    assert hasattr(tf_shim.nn, "relu")
    t = torch.tensor([0.0, -0.0, 0.5, -0.5], requires_grad=True, dtype=torch.float64)      # the shim's relu: torch.relu
    torch.relu(t).sum().backward()
    assert t.grad.tolist() == [0.0, 0.0, 1.0, 0.0], t.grad


def build(dataset, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    mod = load_npe()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "NPE"
    conf.update(hyper)
    sess = tf_shim.Session(seed=0)
    model = mod.NPE(sess, dataset, conf)
    assert {u: list(s) for u, s in model.train_dict.items()} == dataset.seqs      # csr_to_user_dict_bytime
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess


# ------------------------------------------------------------------ inputs
def reserve_windows(seqs, n=3):
    """n users with > W_MAX + 1 items whose first W_MAX + 1 items are disjoint: (user, [r0..r4], target)"""
    out, taken = [], set()
    for u in sorted(seqs):
        s = seqs[u]
        if len(s) >= W_MAX + 2 and not (set(s[:W_MAX + 1]) & taken):
            out.append((u, s[:W_MAX], s[W_MAX]))
            taken |= set(s[:W_MAX + 1])
            if len(out) == n:
                return out
    raise AssertionError("not enough disjoint windows")


def plant_zeros(Pt, Vt, Wt, reserved):
    for u, w, i in reserved:
        Pt[u, 0] = 0.0
        Vt[i, 1] = 0.0
        Wt[w, 2] = [0.125, -0.125, 0.0, 0.25, -0.25]


def make_batches(seqs, n_items, L, steps, reserved, seed):
    """[(users, recents [B, L], items, labels)] per step: windows of the users' sequences (recents oldest first, as the
    sampler delivers them), one label-0 instance per window with an item outside the user's sequence.  Step k holds
    reserved window k; the reserved windows of later steps are kept out in every role."""
    rs = np.random.RandomState(seed)
    win = lambda u, k: (u, seqs[u][k - L:k], seqs[u][k])
    long = [u for u, s in seqs.items() if len(s) >= L + 3]
    out = []
    for k in range(steps):
        barred_users = {u for u, _, _ in reserved[k + 1:]}
        barred_items = {i for _, w, t in reserved[k + 1:] for i in list(w) + [t]}
        free = lambda w: w[0] not in barred_users and not ((set(w[1]) | {w[2]}) & barred_items)
        windows = [w for w in (win(u, j) for u, s in seqs.items() for j in range(L, len(s))) if free(w)]
        ok_long = [u for u in long if u not in {r[0] for r in reserved} and all(free(win(u, L + j)) for j in range(2))]
        u0 = ok_long[rs.randint(len(ok_long))]
        ur, wr, tr = reserved[k]
        u1, r1, i1 = win(u0, L + 1)
        # the reserved window; one user twice, seq[L] the target of its first window and a recent of its second; the
        # second window once more with its first recent replaced by its second (an item twice among the recents)
        pos = [(ur, wr[W_MAX - L:], tr), win(u0, L), (u1, r1, i1), (u1, [r1[1]] + r1[1:], i1)]
        for j in rs.choice(len(windows), B // 2 - len(pos), replace=False):
            pos.append(windows[j])

        def neg(u):
            while True:
                j = int(rs.randint(n_items))
                if j not in seqs[u] and j not in barred_items:
                    return j
        inst = [(u, r, i, 1.0) for u, r, i in pos] + [(u, r, neg(u), 0.0) for u, r, _ in pos]
        inst = [inst[j] for j in rs.permutation(len(inst))]
        users, recents, items = ([p[c] for p in inst] for c in range(3))
        assert len(users) == B
        pat = P.edge_patterns(users, recents, items)
        assert all(pat.values()), pat
        out.append((np.asarray(users, np.int32), np.asarray(recents, np.int32).reshape(B, L),
                    np.asarray(items, np.int32), np.asarray([p[3] for p in inst], np.float32)))
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
        for users, recents, items, labels in batches:
            # the zeros the case is recorded for, on the tables this step looks up, in this width
            zeros = P.zero_counts(*(v.numpy() for v in variables), users, recents, items)
            assert min(zeros) >= 1, (tag, zeros)
            feed = {model.user_input: users, model.item_input: items, model.labels: labels,
                    model.item_input_recent: recents}
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=feed)
            losses.append(float(loss))
            tabs.append(tuple(v.numpy() for v in variables))
        out[tag] = (tabs, np.asarray(losses, np.float64))
        if predict_users is not None:
            out[tag + "_predict"] = _np(model.predict(list(predict_users), None), width)
            out[tag + "_predict_cand"] = _np(model.predict(list(predict_users), [list(c) for c in cand]), width)
    return out


def pack(case, res, init, batches):
    """rows that moved, per table, and their DIFFERENCE from the initial table in float64 (make_golden_fpmc.pack)"""
    init64 = [t.astype(np.float64) for t in init]
    out = {case + "_" + name: np.stack([b[c] for b in batches])
           for c, name in enumerate(("users", "recents", "items", "labels"))}
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
    R = train_matrix(3)
    U, I = R.shape
    seqs = time_orders(R)
    ds = TimedDataset(R, seqs)
    d = HYPER["embedding_size"]
    rs = np.random.RandomState(4219)
    init = [(0.1 * rs.randn(n, d)).astype(np.float32) for n in (U, I, I)]
    reserved = reserve_windows(seqs)
    plant_zeros(*init, reserved)
    by_len = lambda n: [u for u, s in seqs.items() if len(s) == n]
    longer = [u for u, s in seqs.items() if len(s) >= 3]
    assert by_len(1) and by_len(2)
    predict_users = np.asarray(longer[:3] + by_len(2)[:1] + by_len(1)[:1], np.int32)
    cand = np.asarray([[3, 0, I - 1], [7, 7, 1], [0, 1, 2], [I - 1, I - 2, 5], [9, 8, 0]], np.int32)
    ptr = np.zeros(U + 1, np.int64)
    for u, s in seqs.items():
        ptr[u + 1] = len(s)
    ptr = np.cumsum(ptr)
    out = dict(indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32), shape=np.asarray(R.shape, np.int64),
               seq_ptr=ptr, seq=np.asarray([i for u in sorted(seqs) for i in seqs[u]], np.int32),
               P_0=init[0], V_0=init[1], W_0=init[2], predict_users=predict_users, predict_cand=cand,
               zero_users=np.asarray([u for u, _, _ in reserved], np.int32),
               zero_recents=np.asarray([w for _, w, _ in reserved], np.int32),
               zero_items=np.asarray([t for _, _, t in reserved], np.int32),
               reg=np.float64(HYPER["reg"]), learning_rate=np.float64(HYPER["learning_rate"]),
               cases=np.asarray(sorted(P.CASES)))
    gaps = {}
    for k, (case, (loss, learner, L)) in enumerate(sorted(P.CASES.items())):
        hyper = dict(HYPER, loss_function=loss, learner=learner, high_order=L)
        batches = make_batches(seqs, I, L, STEPS.get(case, 2), reserved, seed=700 + k)
        last = case == P.PREDICT_CASE
        res = run_case(ds, init, hyper, batches, predict_users if last else None, cand if last else None)
        out.update(pack(case, res, init, batches))
        if last:
            for tag, _ in WIDTHS:
                out["predict_" + tag] = res[tag + "_predict"]
                out["predict_cand_" + tag] = res[tag + "_predict_cand"]
        gaps[case] = max(np.abs(out["%s_f32_%s" % (case, t)] - out["%s_f64_%s" % (case, t)]).max() for t in P.TABLES)
    path = os.path.join(HERE, "tfgraph_npe.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); fp32 vs fp64 table gaps %s" % (path, os.path.getsize(path),
                                                              {k: "%.3g" % v for k, v in gaps.items()}))


if __name__ == "__main__":
    main()
