"""JCA on the host: the numpy restatement against the reference's own trace and against autograd, the draw rule, the
plugin's surface, the defaults row, the header's limits and the refusals.  No GPU is needed."""
import configparser
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import jca_restatement as P

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "tfgraph_jca.npz"))


def train_of(g):
    U, I = (int(x) for x in g["shape"])
    return sp.csr_matrix((np.ones(len(g["indices"]), np.float32), g["indices"], g["indptr"]), shape=(U, I))


def pairs_of(g, case, s):
    p, n = g["%s_p_%d" % (case, s)], g["%s_n_%d" % (case, s)]
    assert np.array_equal(p[:, 0], n[:, 0])
    return p[:, 0], p[:, 1], n[:, 1]


def _tight(got, want, what, ulps=8):
    """within `ulps` float64 ulps of max(1, the largest value): the two float64 runs differ by the order of their sums"""
    err = np.abs(got - want).max(initial=0)
    bar = ulps * EPS64 * max(1.0, np.abs(want).max(initial=0))
    print("%s: err %.3g (%.1f ulps of the scale)" % (what, err, err / (bar / ulps)))
    assert got.shape == want.shape and err <= bar, (what, err, bar)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", sorted(P.CASES))
def test_the_restatement_follows_the_reference_trace(golden, case):
    """float64 restatement against the float64 trace of the reference's class: every variable after every step, every
    loss, and the ratings in both modes, within 8 float64 ulps of max(1, the largest value).  Achieved by the
    restatement alone: at most 0.5 ulps of that scale on every variable and on the ratings (the sums over up to 157
    terms are taken in another order than torch's), the losses within 64 ulps of their own size."""
    g = golden
    f, ga, learner, reg, num_neg, H, margin, lr = P.CASES[case]
    R = train_of(g)
    U, I = R.shape
    init = P.init_tables(U, I, H, int(g["%s_init_seed" % case]))
    st = P.State(init, np.float64, lr, learner)
    dense = R.toarray().astype(np.float64)
    for s in range(int(g["steps"])):
        rows, cols = g["%s_rows_%d" % (case, s)], g["%s_cols_%d" % (case, s)]
        pairs = pairs_of(g, case, s)
        assert len(pairs[0]) % num_neg == 0
        hinge, regl = P.step(st, dense, rows, cols, pairs, f, ga, margin, reg)
        want_loss = float(g["%s_loss_f64" % case][s])
        assert abs(hinge + regl - want_loss) <= 64 * EPS64 * max(1.0, abs(want_loss)), (s, hinge + regl, want_loss)
        want, _ = P.golden_tables(g, case, init, s)
        for k in P.NAMES:
            _tight(st.T[k], want[k], "%s step %d %s" % (case, s, k))
    users, cand = g["predict_users"], g["predict_cand"]
    full = P.score(st.T, dense, users, f, ga)
    _tight(full, g["predict_%s_f64" % case], "%s ratings" % case)
    _tight(np.take_along_axis(full, cand.astype(np.int64), 1), g["predict_%s_cand_f64" % case], "%s candidates" % case)


def test_the_restatement_follows_the_recorded_epoch(golden):
    """the 4 x 3 blocks of the recorded train_model() epoch at batch_size 48 and H = 50: every block's cost, the logged
    loss (the sum of the last column block's costs), the end tables"""
    g = golden
    f, ga, learner, reg, num_neg, _, margin, lr = P.CASES[P.EPOCH_CASE]
    R = train_of(g)
    U, I = R.shape
    assert int(g["epoch_steps"]) == 12 == (U // P.EPOCH_BATCH + 1) * (I // P.EPOCH_BATCH + 1)
    init = P.init_tables(U, I, P.EPOCH_H, int(g["epoch_init_seed"]))
    st = P.State(init, np.float64, lr, learner)
    dense = R.toarray().astype(np.float64)
    losses, seen_r, seen_c = [], [], []
    for s in range(12):
        rows, cols = g["epoch_rows_%d" % s], g["epoch_cols_%d" % s]
        sub = dense[rows][:, cols]
        pairs = pairs_of(g, "epoch", s)
        assert sub.sum() > 0 and len(pairs[0]) == int(sub.sum()) * num_neg            # every block has a positive
        assert np.all(sub[pairs[0], pairs[1]] == 1) and np.all(sub[pairs[0], pairs[2]] == 0)
        losses.append(sum(P.step(st, dense, rows, cols, pairs, f, ga, margin, reg)))
        if s % 3 == 0:
            seen_r.append(rows)
        if s < 3:
            seen_c.append(cols)
    assert sorted(np.concatenate(seen_r).tolist()) == list(range(U))
    assert sorted(np.concatenate(seen_c).tolist()) == list(range(I))
    assert [len(r) for r in seen_r] == [48, 48, 48, 13] and [len(c) for c in seen_c] == [48, 48, 35]
    np.testing.assert_allclose(losses, g["epoch_loss_f64"], rtol=64 * EPS64)
    logged = sum(losses[s] for s in (2, 5, 8, 11))
    assert abs(logged - float(g["epoch_logged_f64"])) <= 1e-6 * abs(logged)           # the log line prints %f
    want, _ = P.golden_tables(g, "epoch", init, 0)
    for k in P.NAMES:
        _tight(st.T[k], want[k], "epoch end %s" % k)


def test_the_trace_holds_what_the_issue_names(golden):
    g = golden
    assert tuple(g["shape"]) == (157, 131) and len(g["indices"]) == 1135
    deg = np.diff(g["indptr"])
    assert (deg == 0).any() and np.bincount(g["indices"])[0] == 110                   # an empty row, the hub column
    assert g["cases"].tolist() == sorted(P.CASES) and int(g["steps"]) >= 3
    acts = {(c[0], c[1], c[2], c[3] > 0, c[4]) for c in P.CASES.values()}
    assert ("tanh", "tanh", "adam", False, 1) in acts and ("sigmoid", "relu", "gd", True, 1) in acts
    assert ("identity", "elu", "adam", False, 2) in acts
    assert P.EPOCH_H == 50 and any(c[5] % 32 for c in P.CASES.values())
    assert 5 in g["default_rows_0"] and 0 in g["default_cols_0"] and deg[5] == 0
    assert len(g["default_rows_0"]) != len(g["default_cols_0"])
    assert g["predict_users"].shape == (27,) and g["predict_default_f64"].shape == (27, 131)
    assert os.path.getsize(os.path.join(GOLDEN, "tfgraph_jca.npz")) < 1 << 20


@pytest.mark.parametrize("f,ga,reg", [("tanh", "tanh", 0.0), ("sigmoid", "relu", 0.3), ("identity", "elu", 0.1)])
def test_the_restated_gradients_are_autograd_s(f, ga, reg):
    """a 7 x 9 block of a 12 x 15 matrix in float64: the restated gradients plus the regulariser's against
    torch.autograd on the cost written out as the reference writes it"""
    import torch
    rs = np.random.RandomState(11)
    U, I, H, margin = 12, 15, 5, 0.15
    dense = (rs.uniform(size=(U, I)) < 0.3).astype(np.float64)
    dense[3] = 0
    T = {k: v.astype(np.float64) for k, v in P.init_tables(U, I, H, 5, scale=0.5).items()}
    rows, cols = rs.permutation(U)[:7], rs.permutation(I)[:9]
    Rm = sp.csr_matrix(dense)
    a, bp, bn = P.draw_pairs(Rm.indptr, Rm.indices, rows, cols, 99, 1, 0, 0, 2)
    assert len(a) > 10
    hinge, regl, G = P.gradients(T, dense, rows, cols, (a, bp, bn), f, ga, margin, reg)
    tt = {k: torch.tensor(v, requires_grad=True) for k, v in T.items()}
    fn = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu, "elu": torch.nn.functional.elu,
          "identity": lambda x: x}
    Rt = torch.tensor(dense)
    r, c = torch.tensor(rows), torch.tensor(cols)
    hu = fn[ga](Rt[r] @ tt["UV"] + tt["Ub1"])
    u_dec = fn[f](hu @ tt["UW"] + tt["Ub2"])                                       # [Bu, I], as the reference has it
    hi = fn[ga]((Rt[:, c].T @ tt["IV"] + tt["Ib1"]) * tt["I_factor_vector"][0, c][:, None])
    i_dec = fn[f](hi @ tt["IW"] + tt["Ib2"])                                       # [Bi, U]
    D = (u_dec[:, c] + i_dec[:, r].T) / 2.0
    cost1 = torch.clamp(D[a, bn] - D[a, bp] + margin, min=0).sum()
    cost2 = reg * 0.5 * sum((tt[k] ** 2).sum() / 2 for k in P.REGULARISED)
    (cost1 + cost2).backward()
    assert abs(float(cost1.detach()) - hinge) < 1e-12 and abs(float(torch.as_tensor(cost2).detach()) - regl) < 1e-12
    for k in P.NAMES:
        want = tt[k].grad.numpy()
        got = G[k] + (0.5 * reg * T[k] if k in P.REGULARISED else 0.0)
        assert np.abs(got - want).max() < 1e-12, k
    assert np.abs(G["I_factor_vector"]).max() > 0 and np.abs(G["IV"]).max() > 0


# ------------------------------------------------------------------ the draw rule
def _block():
    rs = np.random.RandomState(3)
    dense = (rs.uniform(size=(40, 70)) < 0.2).astype(np.float32)
    dense[7] = 0
    dense[9, :] = 1
    Rm = sp.csr_matrix(dense)
    rows, cols = rs.permutation(40)[:33], rs.permutation(70)[:65]
    for at, u in ((0, 7), (1, 9)):                                 # the empty row and the full row are in the block
        rows[rows == u] = rows[at]
        rows[at] = u
    return dense, Rm, rows, cols


def test_the_draws_are_unobserved_distinct_and_pure():
    dense, Rm, rows, cols = _block()
    sub = dense[rows][:, cols]
    for num_neg in (1, 3):
        a, bp, bn = P.draw_pairs(Rm.indptr, Rm.indices, rows, cols, 2019, 4, 1, 2, num_neg)
        full_row = int(np.flatnonzero(rows == 9)[0])
        assert full_row not in a                                   # no unobserved column: no pairs
        want_pos = np.argwhere(sub[np.arange(33) != full_row].astype(bool))
        assert len(a) == len(want_pos) * num_neg
        assert np.all(sub[a, bp] == 1) and np.all(sub[a, bn] == 0)
        cells = np.stack([a, bp], 1).reshape(-1, num_neg, 2)
        assert np.all(cells == cells[:, :1]) and np.all(np.diff(cells[:, 0, 0] * 512 + cells[:, 0, 1]) > 0)   # row-major
        negs = bn.reshape(-1, num_neg)
        assert all(len(set(r)) == num_neg for r in negs.tolist())
        again = P.draw_pairs(Rm.indptr, Rm.indices, rows, cols, 2019, 4, 1, 2, num_neg)
        assert np.array_equal(again[2], bn)
        # a pure function of the counters: the same cell draws the same negatives whatever else the block holds
        obs = set(np.flatnonzero(sub[a[0]]).tolist())
        assert P.draw_negatives(2019, 4, 1, 2, int(a[0]), int(bp[0]), obs, 65, num_neg) == negs[0].tolist()
        for change in (dict(seed=2020), dict(epoch=5), dict(i=2), dict(j=3)):
            kw = dict(seed=2019, epoch=4, i=1, j=2)
            kw.update(change)
            other = P.draw_pairs(Rm.indptr, Rm.indices, rows, cols, kw["seed"], kw["epoch"], kw["i"], kw["j"], num_neg)
            assert np.array_equal(other[1], bp) and not np.array_equal(other[2], bn)


def test_the_counting_fallback_takes_over_after_the_rejections():
    """a row of 512 columns with 3 unobserved: 64 rejections are likely, and both paths give unobserved, distinct
    negatives"""
    obs = set(range(512)) - {5, 77, 400}
    hit = set()
    for bp in range(40):
        got = P.draw_negatives(1, 1, 0, 0, 0, bp, obs, 512, 3)
        assert sorted(got) == [5, 77, 400]
        hit.add(tuple(got))
    assert len(hit) > 1


def test_the_draws_are_uniform_over_the_unobserved_columns():
    """the first negative of 4,000 positives' counters over a block row with five unobserved columns, seed fixed:
    Pearson's statistic against the 1 - 1e-6 quantile of chi-square with 4 degrees of freedom.  The survival function
    of 4 degrees is exp(-x / 2) (1 + x / 2); the quantile is solved from it, not tuned."""
    lo, hi = 0.0, 200.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if math.exp(-mid / 2) * (1 + mid / 2) > 1e-6 else (lo, mid)
    bound = hi
    assert 33.3 < bound < 33.5
    free = [2, 3, 11, 17, 30]
    obs = set(range(32)) - set(free)
    counts = dict.fromkeys(free, 0)
    n = 4000
    for q in range(n):
        (neg,) = P.draw_negatives(2019, 1 + q // 500, (q // 50) % 10, 0, q % 50, sorted(obs)[q % len(obs)], obs, 32, 1)
        counts[neg] += 1
    chi2 = sum((c - n / 5) ** 2 / (n / 5) for c in counts.values())
    print("chi-square %.3f against %.3f" % (chi2, bound))
    assert chi2 < bound


# ------------------------------------------------------------------ the plugin on the host
def test_find_recommender_resolves_jca():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import AbstractRecommender
    cls = find_recommender("JCA")
    assert cls.__module__ == "neurec_amd.model.general_recommender.JCA" and issubclass(cls, AbstractRecommender)
    doc = sys.modules[cls.__module__].__doc__
    assert "As the reference" in doc and "Deviations" in doc
    for quirk in ("corruption_level", "outside the inner loop", "int(num_users / batch_size) + 1", "afresh each epoch",
                  "epochs run from 1", "whole matrix", "both modes"):
        assert quirk in doc, quirk
    keys = re.findall(r'conf\["(\w+)"\]', inspect.getsource(cls.__init__))
    assert keys == ["hidden_neuron", "learning_rate", "learner", "reg", "epochs", "batch_size", "verbose", "f_act", "g_act",
                    "margin", "corruption_level", "init_method", "stddev", "num_neg"]


def test_the_defaults_row_equals_the_properties_file(tmp_path):
    from neurec_amd import defaults
    ref = configparser.ConfigParser()
    ref.optionxform = str
    assert ref.read(os.path.join(GOLDEN, "neurec_conf", "conf", "JCA.properties"))
    want = dict(ref["hyperparameters"])
    assert dict(defaults.MODELS["JCA"]) == want and [k for k, _ in defaults.MODELS["JCA"]] == list(want)
    path = defaults.write_default_configs(str(tmp_path))
    from neurec_amd.util.configurator import Configurator
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=JCA", "--num_neg=2"])
    finally:
        os.chdir(cwd)
    assert (conf["hidden_neuron"], conf["batch_size"], conf["num_neg"], conf["epochs"]) == (50, 256, 2, 200)
    assert (conf["f_act"], conf["g_act"], conf["learner"], conf["margin"], conf["reg"]) == ("tanh", "tanh", "adam", 0.15, 0)


class _Engine:
    dev = "cpu"

    def __init__(self, empty=()):
        self.calls, self.empty = [], set(empty)

    def pairs(self, rows, cols, epoch, i, j):
        self.calls.append((epoch, i, j, np.asarray(rows).copy(), np.asarray(cols).copy()))
        return (i, j)

    def step(self, rows, cols, pairs, loss_out):
        i, j = pairs
        loss_out[0], loss_out[1] = (0.0, 0.0) if (i, j) in self.empty else (float(10 * i + j), 0.25)

    def encode_items(self):
        self.calls.append("encode")


def test_the_plugin_walks_the_blocks_and_logs_the_reference_s_lines():
    """train_model() on a recording engine: epochs from 1, fresh permutations per epoch, int(n / B) + 1 batches with the
    last one short (empty when n is a multiple of B), and the logged loss = the sum of the LAST column block's losses"""
    from neurec_amd.model.general_recommender.JCA import JCA
    lines = []
    model = JCA.__new__(JCA)
    model.logger = type("L", (), {"info": staticmethod(lambda m: lines.append(str(m)))})()
    model.evaluator = type("E", (), {"metrics_info": staticmethod(lambda: "metrics"),
                                     "evaluate": staticmethod(lambda m: "recorded")})()
    model.engine = _Engine()
    model.num_users, model.num_items, model.batch_size, model.num_epochs, model.verbose = 10, 8, 4, 2, 2
    np.random.seed(5)
    model.train_model()
    blocks = [c for c in model.engine.calls if c != "encode"]
    assert [(e, i, j) for e, i, j, _, _ in blocks] == [(e, i, j) for e in (1, 2) for i in range(3) for j in range(3)]
    assert [len(r) for _, _, j, r, _ in blocks if j == 0] == [4, 4, 2] * 2
    assert [len(c) for _, i, _, _, c in blocks if i == 0] == [4, 4, 0] * 2           # 8 items in batches of 4: an empty one
    first = np.concatenate([r for e, _, j, r, _ in blocks if e == 1 and j == 0])
    second = np.concatenate([r for e, _, j, r, _ in blocks if e == 2 and j == 0])
    assert sorted(first.tolist()) == sorted(second.tolist()) == list(range(10)) and not np.array_equal(first, second)
    assert model.engine.calls.count("encode") == 1
    assert lines[0] == "metrics" and len(lines) == 4 and lines[3] == "epoch 2:\trecorded"
    total = sum(10 * i + 2 + 0.25 for i in range(3))
    for e, line in ((1, lines[1]), (2, lines[2])):
        m = re.fullmatch(r"\[iter (\d+) : loss : ([0-9.]+), time: ([0-9.]+)\]", line)
        assert m and int(m.group(1)) == e and float(m.group(2)) == pytest.approx(total)


def test_the_refusals_name_the_key_and_the_range(monkeypatch):
    from neurec_amd.jca import check_config, check_train_values
    ok = dict(hidden_neuron=50, batch_size=256, num_neg=1, f_act="tanh", g_act="tanh", learner="adam", margin=0.15,
              reg=0.0, learning_rate=0.001)
    check_config(**ok)
    check_config(**dict(ok, hidden_neuron=128, batch_size=512, num_neg=8, f_act="elu", g_act="identity", learner="gd",
                        margin=0.0))
    for change, exc, text in ((dict(hidden_neuron=129), NotImplementedError, r"hidden_neuron=129 is not supported \(1 to 128\)"),
                              (dict(hidden_neuron=0), NotImplementedError, r"hidden_neuron=0"),
                              (dict(batch_size=513), NotImplementedError, r"batch_size=513 is not supported \(1 to 512\)"),
                              (dict(num_neg=9), NotImplementedError, r"num_neg=9 is not supported \(1 to 8\)"),
                              (dict(num_neg=0), NotImplementedError, r"num_neg=0"),
                              (dict(f_act="softmax"), NotImplementedError, r"f_act='softmax' is not supported .*softmax needs"),
                              (dict(g_act="selu"), NotImplementedError, r"g_act='selu' is not supported .*selu is left out"),
                              (dict(learner="adagrad"), NotImplementedError, r"learner='adagrad' is not supported \(one of adam, gd\)"),
                              (dict(margin=-0.1), ValueError, r"margin=-0.1 is not supported \(margin >= 0\)"),
                              (dict(reg=-1.0), ValueError, r"reg=-1.0 is not supported \(reg >= 0\)"),
                              (dict(learning_rate=0.0), ValueError, r"learning_rate=0.0 is not supported \(learning_rate > 0\)")):
        with pytest.raises(exc, match=text):
            check_config(**dict(ok, **change))
    rated = sp.csr_matrix(np.asarray([[1.0, 0.0, 4.0], [0.0, 1.0, 0.0]], np.float32))
    with pytest.raises(ValueError, match=r"the train matrix holds the value 4.0; only stored values of 1"):
        check_train_values(rated)
    from neurec_amd.model.general_recommender.JCA import JCA
    from neurec_amd import parallel
    model = JCA.__new__(JCA)
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)
    with pytest.raises(NotImplementedError, match="JCA runs on one GPU"):
        model.build_graph()


def test_the_header_s_limits_are_the_python_constants_and_the_entries_refuse_by_name():
    import ctypes as C
    from neurec_amd import _lib, jca
    with open(os.path.join(ROOT, "include", "neurec_hip.h")) as fh:
        header = fh.read()
    macros = {k: int(v) for k, v in re.findall(r"#define NRHIP_JCA_(\w+) (\d+)", header)}
    assert (macros["MAX_H"], macros["MAX_BATCH"], macros["MAX_NEG"]) == (jca.MAX_H, jca.MAX_BATCH, jca.MAX_NEG) == \
        (128, 512, 8)
    assert [macros["ACT_" + a.upper()] for a in jca.ACTIVATIONS] == list(range(5))
    assert jca.NAMES == P.NAMES
    sizes = (C.c_int64 * 4)()
    out = C.cast(sizes, C.c_void_p)
    _lib.call("nrhip_jca_workspace", 157, 131, 50, 48, 2, out)
    assert sizes[0] == 5 * 48 * 50 + 2 * 48 * 48 and sizes[1] >= 48 * 48 + 48 * 16 + 48 and sizes[3] == 48 * 48 * 2
    for args, text in (((157, 131, 129, 48, 1), r"hidden_neuron 129 outside 1..128"),
                       ((157, 131, 50, 513, 1), r"batch_size 513 outside 1..512"),
                       ((157, 131, 50, 48, 9), r"num_neg 9 outside 1..8")):
        with pytest.raises(NotImplementedError, match=text):
            _lib.call("nrhip_jca_workspace", *args, out)
    for entry in ("nrhip_jca_pairs", "nrhip_jca_step"):
        with pytest.raises(ValueError, match="null argument"):
            _lib.call(entry, None, None)
    a = _lib.JcaArgs()
    a.n_users, a.n_items, a.H, a.batch_size, a.num_neg, a.f_act, a.g_act = 157, 131, 50, 48, 1, 7, 1
    with pytest.raises(NotImplementedError, match=r"jca_step: unknown activation \(f_act 7"):
        _lib.call("nrhip_jca_step", C.byref(a), None)
