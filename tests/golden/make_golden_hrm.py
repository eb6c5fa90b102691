"""Golden HRM trace produced by the REFERENCE's own HRM class (model/sequential_recommender/HRM.py).

The class is loaded whole and unchanged with oracle/ref_models._load_file and runs under oracle/tf_shim.py, with the
module stand-ins make_golden_fpmc.py registers for FPMC.  The shim lacks tf.reduce_max: attach_ops() adds it as
torch.amax over the axis, whose gradient is TF's _MinOrMaxGrad rule (the derivative split equally among the inputs equal
to the maximum; checked in attach_ops).  The maker drives `sess.run((model.loss, model.optimizer), feed_dict)` itself;
train_model() is not called.  predict() is the reference's.

    python tests/golden/make_golden_hrm.py              # needs the reference tree

Writes tests/golden/tfgraph_hrm.npz:
  indptr / indices / shape     the train pattern: make_golden_fossil.train_matrix(3) (157 x 131; users with 1, 2, 3 and
                               4 items exist)
  seq_ptr / seq                every user's items by time: a seeded permutation of the row
  P_0 / V_0                    the initial tables (0.1 randn) with PLANTED TIES: for each of three reserved windows
                               (user u, recents a b c) column 0 holds 0.25 in P[u] and in all three recents (the user
                               ties with the session row under max and under avg, and the recents tie three ways),
                               column 1 holds 0.1875 in b and c and -0.125 in a (a two-way session tie); dyadic values,
                               so float32 and float64 tie alike
  tie_users / tie_recents      the reserved windows [3] / [3, 3]; window k is held out of every batch before step k, in
                               every role, so that its rows still hold their initial values when step k looks them up
  <case>_users/_recents/_items/_labels   the batches [steps, B] ([steps, B, L] recents, oldest first)
  <case>_rows_{P,V}            the rows of that table that differ from its initial value at any step, in either width
  <case>_{f32,f64}_{P,V}       [steps, len(rows), d]: those rows after each step MINUS their initial value, in float64;
  <case>_{f32,f64}_loss [steps]   the fetched (pre-update) loss
  predict_users, predict_{f32,f64}, predict_cand, predict_cand_{f32,f64}
                               predict() rows after the last step of the case `ce_adam_max_max` (L = 3), full and
                               candidate mode: users with |R_u| >= 3, with |R_u| = 2 (pooled over 1) and |R_u| = 1
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
import hrm_restatement as P                   # noqa: E402

HYPER = dict(epochs=1, batch_size=64, embedding_size=16, reg_mf=0.01, learning_rate=0.01, learner="adam",
             pre_agg="max", session_agg="max", high_order=3, num_neg=4, loss_function="cross_entropy",
             init_method="normal", stddev=0.01, verbose=1, topk=20)
STEPS = {"ce_adam_max_max": 3}                # every other case: 2
B = 60


def load_hrm():
    """the reference module model/sequential_recommender/HRM.py, executed under the shim (make_golden_fpmc.load_fpmc's
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
        mod = rm._load_file("model.sequential_recommender.HRM",
                            os.path.join(rm.REF, "model", "sequential_recommender", "HRM.py"))
        sys.modules.pop("model.sequential_recommender.HRM", None)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        tf_shim.uninstall(saved_tf)


def attach_ops():
    """tf.reduce_max, which the shim lacks: torch.amax over the axis.  Its gradient divides the derivative equally
    among the tied inputs, as TF's _MinOrMaxGrad does — checked here on a two-way and a three-way tie."""
    import torch
    if not hasattr(tf_shim, "reduce_max"):
        def reduce_max(x, axis=None, keepdims=False, name=None, keep_dims=None):
            ax = tf_shim._axes(axis)
            kd = True if (keepdims or keep_dims) else False
            return tf_shim.Tensor(lambda a: torch.amax(a) if ax is None else torch.amax(a, dim=ax, keepdim=kd), [x])
        tf_shim.reduce_max = reduce_max
    t = torch.tensor([[1.0, 1.0, 0.5], [2.0, 2.0, 2.0]], requires_grad=True, dtype=torch.float64)
    torch.amax(t, dim=1).sum().backward()
    assert t.grad.tolist() == [[0.5, 0.5, 0.0], [1 / 3, 1 / 3, 1 / 3]], t.grad
    for name in ("multiply", "reduce_sum", "reduce_mean", "concat", "expand_dims", "placeholder"):
        assert hasattr(tf_shim, name), name


def build(dataset, hyper, width):
    tf_shim.set_float(width)
    tf_shim.reset_default_graph()
    mod = load_hrm()
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf["recommender"] = "HRM"
    conf.update(hyper)
    sess = tf_shim.Session(seed=0)
    model = mod.HRM(sess, dataset, conf)
    assert {u: list(s) for u, s in model.train_dict.items()} == dataset.seqs      # csr_to_user_dict_bytime
    model.build_graph()
    sess.run(tf_shim.global_variables_initializer())
    return model, sess


# ------------------------------------------------------------------ inputs
def reserve_windows(seqs, n=3):
    """n users with >= 4 items whose first three items are disjoint: (user, [a, b, c]) — the windows the ties are
    planted in; the L = 2 cases use (b, c), the L = 1 cases c"""
    out, taken = [], set()
    for u in sorted(seqs):
        s = seqs[u]
        if len(s) >= 5 and not (set(s[:4]) & taken):          # the window's target s[3] too: in no other window
            out.append((u, s[:3]))
            taken |= set(s[:4])
            if len(out) == n:
                return out
    raise AssertionError("not enough disjoint windows")


def plant_ties(Pt, Vt, reserved):
    for u, (a, b, c) in reserved:
        Pt[u, 0] = Vt[a, 0] = Vt[b, 0] = Vt[c, 0] = 0.25
        Vt[b, 1] = Vt[c, 1] = 0.1875
        Vt[a, 1] = -0.125


def make_batches(seqs, n_items, L, steps, reserved, seed):
    """[(users, recents [B, L], items, labels)] per step: windows of the users' sequences (recents oldest first, as the
    sampler delivers them), one label-0 instance per window with an item outside the user's sequence.  Step k holds
    reserved window k; the reserved windows of later steps are kept out in every role."""
    rs = np.random.RandomState(seed)
    win = lambda u, k: (u, seqs[u][k - L:k], seqs[u][k])
    long = [u for u, s in seqs.items() if len(s) >= L + 3]
    out = []
    for k in range(steps):
        barred_users = {u for u, _ in reserved[k + 1:]}
        barred_items = {i for _, w in reserved[k + 1:] for i in w}
        free = lambda w: w[0] not in barred_users and not ((set(w[1]) | {w[2]}) & barred_items)
        windows = [w for w in (win(u, j) for u, s in seqs.items() for j in range(L, len(s))) if free(w)]
        ok_long = [u for u in long if all(free(win(u, L + j)) for j in range(2))]
        u0 = ok_long[rs.randint(len(ok_long))]
        ur, wr = reserved[k]
        # the reserved window; one user twice, seq[L] the target of its first window and a recent of its second
        pos = [(ur, wr[3 - L:], seqs[ur][3]), win(u0, L), win(u0, L + 1)]
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
    pre_max, ses_max = hyper["pre_agg"] == "max", hyper["session_agg"] == "max" and hyper["high_order"] > 1
    for tag, width in WIDTHS:
        _reset_recorders()
        model, sess = build(ds, hyper, width)
        for var, t in zip((model.user_embeddings, model.item_embeddings), init):
            var.load(t)
        tabs, losses = [], []
        for users, recents, items, labels in batches:
            # the ties the case is recorded for, on the tables this step looks up, in this width
            n_sess, n_pre = P.tie_counts(model.user_embeddings.numpy(), model.item_embeddings.numpy(), users, recents,
                                         hyper["pre_agg"], hyper["session_agg"])
            assert (not ses_max or n_sess >= 1) and (not pre_max or n_pre >= 1), (tag, n_sess, n_pre)
            feed = {model.user_input: users, model.item_input: items, model.labels: labels,
                    model.item_input_recent: recents if hyper["high_order"] > 1 else recents.reshape(-1)}
            loss, _ = sess.run((model.loss, model.optimizer), feed_dict=feed)
            losses.append(float(loss))
            tabs.append(tuple(v.numpy() for v in (model.user_embeddings, model.item_embeddings)))
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
    rs = np.random.RandomState(4211)
    init = [(0.1 * rs.randn(n, d)).astype(np.float32) for n in (U, I)]
    reserved = reserve_windows(seqs)
    plant_ties(init[0], init[1], reserved)
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
               P_0=init[0], V_0=init[1], predict_users=predict_users, predict_cand=cand,
               tie_users=np.asarray([u for u, _ in reserved], np.int32),
               tie_recents=np.asarray([w for _, w in reserved], np.int32),
               reg_mf=np.float64(HYPER["reg_mf"]), learning_rate=np.float64(HYPER["learning_rate"]),
               cases=np.asarray(sorted(P.CASES)))
    gaps = {}
    for k, (case, (loss, learner, pre, ses, L)) in enumerate(sorted(P.CASES.items())):
        hyper = dict(HYPER, loss_function=loss, learner=learner, pre_agg=pre, session_agg=ses, high_order=L)
        batches = make_batches(seqs, I, L, STEPS.get(case, 2), reserved, seed=500 + k)
        last = case == P.PREDICT_CASE
        res = run_case(ds, init, hyper, batches, predict_users if last else None, cand if last else None)
        out.update(pack(case, res, init, batches))
        if last:
            for tag, _ in WIDTHS:
                out["predict_" + tag] = res[tag + "_predict"]
                out["predict_cand_" + tag] = res[tag + "_predict_cand"]
        gaps[case] = max(np.abs(out["%s_f32_%s" % (case, t)] - out["%s_f64_%s" % (case, t)]).max() for t in P.TABLES)
    path = os.path.join(HERE, "tfgraph_hrm.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); fp32 vs fp64 table gaps %s" % (path, os.path.getsize(path),
                                                              {k: "%.3g" % v for k, v in gaps.items()}))


if __name__ == "__main__":
    main()
