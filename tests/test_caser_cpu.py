"""Caser without a GPU: the numpy restatement (tests/caser_restatement.py) against the trace of the reference class, the
plugin's sequences and feeds against the recorded epoch, the feature order, tied maxima, the pad-target rule, the
creation order, the refusals and defaults, the maker's attached shim ops and the C entries' bounds."""
import configparser
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import caser_restatement as P
from caser_restatement import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISSUE_CASES = {"first": (8, 5, 3, 3, 4, 4, 0.001, 0.0), "second": (50, 5, 3, 3, 4, 16, 0.001, 0.5),
               "third": (3, 1, 1, 1, 1, 1, 0.0, 0.0), "fourth": (12, 7, 2, 5, 3, 5, 0.0, 0.3)}


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_caser")


def case_init(g, case):
    d, L, T, N, nv, nh, l2, rate = CASES["first" if case == "epoch" else case]
    U, I = (int(x) for x in g["shape"])
    return P.init_tables(U, I, d, L, nv, nh, seed=int(g[case + "_init_seed"]))


def case_inputs(g, case):
    d, L, T, N, nv, nh, l2, rate = CASES[case]
    S = len(g[case + "_seq"])
    feeds = [tuple(g["%s_%s" % (case, k)][s] for k in ("users", "seq", "pos", "neg")) for s in range(S)]
    masks = [g[case + "_mask"][s] for s in range(S)] if rate else None
    return P.table_names(L), case_init(g, case), feeds, masks


def golden_table(g, case, name, s, init=None):
    """the variable after step s + 1 of the float64 trace: initial value + stored difference"""
    init = case_init(g, case) if init is None else init
    return init[name].astype(np.float64) + g["%s_f64_%s" % (case, name)][s].astype(np.float64)


def test_the_cases_cover_the_issue_s_list(golden):
    g = golden
    assert CASES == ISSUE_CASES and P.PREDICT_CASE == "second"
    assert sorted(g["cases"].tolist()) == sorted(CASES) and tuple(g["shape"]) == (157, 131) and int(g["batch_step"]) == 20
    I = int(g["shape"][1])
    for case, (d, L, T, N, nv, nh, l2, rate) in CASES.items():
        users, seq, pos, neg = (g["%s_%s" % (case, k)] for k in ("users", "seq", "pos", "neg"))
        assert users.shape == (3, 20) and seq.shape == (3, 20, L) and pos.shape == (3, 20, T) and neg.shape == (3, 20, N)
        assert (pos != I).all() and (neg != I).all()            # no pad target: the shim would raise as TF-CPU does
        n_pad = (seq == I).sum(2)
        real = seq != I                                          # pre-padding: the real positions are a suffix
        assert (real[:, :, 1:] >= real[:, :, :-1]).all()
        for s in range(3):                                       # every kind of row in every step
            assert (n_pad[s] == 0).any() and (n_pad[s] == 1).any() and (n_pad[s] >= max(1, (L + 1) // 2)).any()
            assert np.bincount(users[s]).max() >= 2              # a user twice
        if case == "fourth":
            assert (n_pad > 0).mean() > 0.5                      # most rows front-padded
        if rate:
            m = g[case + "_mask"]
            assert m.shape == (3, 20, nv * d + nh * L) and m.dtype == np.uint8 and set(np.unique(m)) == {0, 1}
        else:
            assert case + "_mask" not in g
    assert 1 <= len(g["epoch_seq"]) <= 40 and (g["epoch_pos"][0] == I).sum() + (g["epoch_pos"][1:-1] == I).sum() > 0


@pytest.mark.parametrize("ties", ["even", "first"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_restatement_equals_the_f64_trace(golden, case, ties):
    """losses and every variable after every step, in float64, with TF's even split and with the kernel's first
    maximum.  The stored differences are float32 (2^-24 of ~3e-3 lost); beyond that 1e-11 for float64 rounding noise
    under Adam's lr / eps = 1e5"""
    g = golden
    d, L, T, N, nv, nh, l2, rate = CASES[case]
    names, init, feeds, masks = case_inputs(g, case)
    tabs, losses = P.train(init, feeds, int(g["shape"][1]), nv, nh, rate, l2, masks, ties, np.float64, float(g["lr"]))
    assert np.abs(np.asarray(losses) - g[case + "_loss_f64"]).max() < 1e-12
    for s in range(len(feeds)):
        for n in names:
            want = golden_table(g, case, n, s, init)
            lost = 2.0 ** -24 * np.abs(g["%s_f64_%s" % (case, n)][s]).max()
            assert np.abs(tabs[s][n] - want).max() <= lost + 1e-11, (case, ties, s, n)


def test_rows_outside_the_batches_never_move_without_a_regulariser(golden):
    """seq_item_embeddings takes ApplyAdam over every row, and a row with a zero gradient and zero slots stays.  (The
    sparse and the dense form of Adam are the same algebra — m b1 + g (1 - b1) against m + (g - m) (1 - b1) — and both
    sweep every row, so swapping them moves the trace by rounding only, 1e-10 here: no test can tell them apart.)"""
    g = golden
    case = "fourth"
    d, L, T, N, nv, nh, l2, rate = CASES[case]
    names, init, feeds, masks = case_inputs(g, case)
    I = int(g["shape"][1])
    swapped = {"seq_item_embeddings"}
    tabs, _ = P.train(init, feeds, I, nv, nh, rate, l2, masks, "even", np.float64, float(g["lr"]), sparse=swapped)
    err = {n: np.abs(tabs[-1][n] - golden_table(g, case, n, 2, init)).max() for n in P.TABLES}
    assert max(err.values()) < 1e-8, err
    seen = np.unique(np.concatenate([f[1].reshape(-1) for f in feeds]))
    still = np.setdiff1d(np.arange(I), seen)
    assert len(still) and not g[case + "_f64_seq_item_embeddings"][:, still].any()


def test_the_float32_restatement_stays_within_the_rule_of_the_trace(golden):
    """the rule the GPU tests use, on the restatement in float32: 4x the reference's own f32-to-f64 distance plus
    1e-5 max|want|"""
    g = golden
    case = "second"
    d, L, T, N, nv, nh, l2, rate = CASES[case]
    names, init, feeds, masks = case_inputs(g, case)
    tabs, _ = P.train(init, feeds, int(g["shape"][1]), nv, nh, rate, l2, masks, "first", np.float32, float(g["lr"]))
    for s in range(len(feeds)):
        for n in names:
            w64 = golden_table(g, case, n, s, init)
            tol = 4 * float(g["%s_gap_%s" % (case, n)][s]) + 1e-5 * np.abs(w64).max()
            assert np.abs(tabs[s][n] - w64).max() <= tol, (s, n)


def test_predict_leaves_the_item_biases_out(golden):
    """predict() of the reference after the trained case, full and candidate mode: p . item_embeddings^T (Caser.py:122)"""
    g = golden
    case = P.PREDICT_CASE
    d, L, T, N, nv, nh, l2, rate = CASES[case]
    names, init, feeds, masks = case_inputs(g, case)
    I = int(g["shape"][1])
    tabs, _ = P.train(init, feeds, I, nv, nh, rate, l2, masks, "even", np.float64, float(g["lr"]))
    assert np.abs(tabs[-1]["item_biases"]).max() > 0.01
    users = g["predict_users"]
    ptr, seq = g["seq_ptr"], g["seq"]
    rows = np.full((len(users), L), I, np.int32)
    for r, u in enumerate(users):
        cut = seq[max(ptr[u], ptr[u + 1] - L):ptr[u + 1]]
        rows[r, L - len(cut):] = cut
    got = P.scores(tabs[-1], users, rows, I, nv, nh)
    tol = 2.0 ** -24 * np.abs(got).max() + 1e-10               # the reference's predict() rounds its rows to float32
    assert np.abs(got - g["predict_f64"]).max() <= tol
    cand = np.stack([got[k][c] for k, c in enumerate(g["predict_cand"])])
    assert np.abs(cand - g["predict_cand_f64"]).max() <= tol
    with_bias = got + tabs[-1]["item_biases"]
    assert np.abs(with_bias - g["predict_f64"]).max() > 0.01


# ------------------------------------------------------------------ the graph's fine print
def _small(seed=3, U=6, I=9, d=4, L=4, T=2, N=2, nv=3, nh=2):
    return U, I, d, L, T, N, nv, nh, {k: v.astype(np.float64) for k, v in P.init_tables(U, I, d, L, nv, nh, seed).items()}


def test_the_vertical_features_are_column_major_in_the_embedding_dimension():
    """the reshape of (b, 1, d, nv) to (b, nv d): feature j nv + c, not c d + j; the heights follow in order"""
    U, I, d, L, T, N, nv, nh, tab = _small()
    seq = np.asarray([[I, 2, 5, 7], [1, 1, 3, 8]])
    p, s = P.forward(tab, [0, 1], seq, I, nv, nh)
    E = np.concatenate([tab["seq_item_embeddings"], np.zeros((1, d))])[seq]
    for b in range(2):
        for j in range(d):
            for c in range(nv):
                want = tab["conv_v_bias"][c] + (E[b, :, j] * tab["conv_v_kernel"][:, c]).sum()
                assert abs(s["x"][b, j * nv + c] - want) < 1e-14
        for i in range(1, L + 1):
            K, bh = tab["conv_h%d_kernel" % i], tab["conv_h%d_bias" % i]
            for c in range(nh):
                vals = [max(0.0, bh[c] + (E[b, q:q + i, :] * K[:, :, c]).sum()) for q in range(L - i + 1)]
                assert abs(s["x"][b, nv * d + (i - 1) * nh + c] - max(vals)) < 1e-14
    # the all-pad window of row 0 takes part in the max: relu(bias) where every real window is below it
    tab["conv_h1_bias"][:] = 50.0
    tab["conv_h1_kernel"], tab["seq_item_embeddings"] = -np.abs(tab["conv_h1_kernel"]), np.abs(tab["seq_item_embeddings"])
    p2, s2 = P.forward(tab, [0, 1], seq, I, nv, nh)
    assert (s2["x"][0, nv * d:nv * d + nh] == 50.0).all() and (s2["x"][1, nv * d:nv * d + nh] < 50.0).all()


def test_tied_maxima_the_even_split_equals_the_first_maximum():
    """all-pad windows tie at relu(bias), a repeated item ties under height 1: TF's even split and the kernel's first
    maximum give the same gradients, because the tied windows hold the same inputs"""
    U, I, d, L, T, N, nv, nh, tab = _small(seed=5)
    for i in range(1, L + 1):
        tab["conv_h%d_bias" % i] = np.abs(tab["conv_h%d_bias" % i]) + 3.0    # the pad windows win the max
    users = np.asarray([0, 1, 2, 2])
    seq = np.asarray([[I, I, I, 4], [I, I, 6, 6], [5, 5, 5, 5], [I, I, I, I]])
    pos = np.asarray([[1, 2], [3, 3], [0, 8], [4, 5]])
    neg = np.asarray([[7, 0], [1, 2], [2, 2], [6, 7]])
    _, s = P.forward(tab, users, seq, I, nv, nh, ties="even")
    shares = np.concatenate([sv[2].reshape(-1) for sv in s["saved"]])
    assert ((shares > 0) & (shares < 1)).sum() >= 8                         # ties are there
    tab["conv_h1_bias"] = -np.abs(tab["conv_h1_bias"])                       # ... and a repeated item under height 1
    tab["conv_h1_kernel"] = np.abs(tab["conv_h1_kernel"])
    tab["seq_item_embeddings"][5] = np.abs(tab["seq_item_embeddings"][5]) + 9.0
    _, s = P.forward(tab, users, seq, I, nv, nh, ties="even")
    assert (s["saved"][0][2][2] == 0.25).all() and (s["saved"][0][1][2] > 0).all()
    le, Ge = P.gradients(tab, users, seq, pos, neg, I, nv, nh, l2_reg=0.01, ties="even")
    lf, Gf = P.gradients(tab, users, seq, pos, neg, I, nv, nh, l2_reg=0.01, ties="first")
    assert le == lf
    for k in Ge:
        assert np.abs(Ge[k] - Gf[k]).max() <= 1e-15 * max(1.0, np.abs(Ge[k]).max()), k
    assert np.abs(Ge["conv_h1_kernel"]).max() > 0 and np.abs(Ge["conv_h2_bias"]).max() > 0


def test_a_pad_target_has_logit_zero_and_no_gradient_and_stays_in_the_mean():
    U, I, d, L, T, N, nv, nh, tab = _small(seed=7)
    users = np.asarray([0, 1, 1])
    seq = np.asarray([[I, I, I, 4], [1, 2, 3, 4], [I, 2, 6, 6]])
    pos = np.asarray([[I, 2], [3, 3], [0, 8]])
    neg = np.asarray([[7, 0], [1, 2], [2, 2]])
    loss, G = P.gradients(tab, users, seq, pos, neg, I, nv, nh)
    # the same batch with the pad target's slot given to a real item whose row and bias are zero
    tab2 = {k: v.copy() for k, v in tab.items()}
    tab2["item_embeddings"][5], tab2["item_biases"][5] = 0.0, 0.0
    pos2 = pos.copy()
    pos2[0, 0] = 5
    loss2, G2 = P.gradients(tab2, users, seq, pos2, neg, I, nv, nh)
    assert abs(loss - loss2) < 1e-15                           # logit 0, in the mean over B T
    term = -np.log(0.5 + 1e-24) / pos.size
    keep = np.ones_like(pos, bool)
    keep[0, 0] = False
    assert loss > term
    assert not G["item_embeddings"][5].any() and G2["item_embeddings"][5].any()   # the real item takes a gradient
    for k in G:
        if k not in ("item_embeddings", "item_biases"):
            assert np.abs(G[k] - G2[k]).max() < 1e-15, k       # a zero row hands nothing back to p
    # the pad row of the sequence table: row 0's three pad positions hand nothing to any table row
    assert G["seq_item_embeddings"].shape == (I, d)


def test_the_float32_loss_tail_saturates():
    """sigmoid exactly 1 in float32 beyond about 17: a negative there costs exactly -log(1e-24) with gradient 0; a
    positive at -100 has sigmoid 0 and the same; float64 does neither"""
    cap = -np.log(np.float32(1e-24))
    loss, dp, dn = P.loss_tail(np.asarray([[-100.0]]), np.asarray([[30.0]]), np.float32)
    assert loss.dtype == np.float32 and loss == np.float32(cap + cap) and dp[0, 0] == 0 and dn[0, 0] == 0
    loss64, dp64, dn64 = P.loss_tail(np.asarray([[-100.0]]), np.asarray([[30.0]]), np.float64)
    assert abs(loss64 - (55.262 + 30.0)) < 0.01 and -1e-15 < dp64[0, 0] < 0 and dn64[0, 0] > 0.9
    loss, dp, dn = P.loss_tail(np.asarray([[-30.0]]), np.asarray([[-30.0]]), np.float32)
    assert abs(float(loss) - 30.0) < 1e-4 and abs(dp[0, 0] + 1.0) < 1e-6 and 0 < dn[0, 0] < 1e-12


# ------------------------------------------------------------------ the sequences and the feeds
def _user_dict(g):
    ptr, seq = g["seq_ptr"], g["seq"]
    return {u: seq[ptr[u]:ptr[u + 1]].tolist() for u in range(len(ptr) - 1) if ptr[u + 1] > ptr[u]}


def test_the_sequences_and_epoch_feeds_are_bit_equal_to_the_recorded_epoch(golden):
    """the reference's train_model() from the same seed with the same stand-in sampler on numpy's stream:
    _sample_negative's draws first, then the shuffle"""
    from neurec_amd.model.sequential_recommender.Caser import epoch_feeds, generate_sequences
    g = golden
    I, B = int(g["shape"][1]), int(g["batch_epoch"])
    d, L, T, N, nv, nh, l2, _ = CASES["first"]
    train = _user_dict(g)
    users_list, seq_list, pos_list, test_seq = generate_sequences(train, I, L, T)
    for u, items in train.items():
        assert list(test_seq[u]) == ([I] * L + items)[-L:]                # the last L of the first window
        mine = [k for k, v in enumerate(users_list) if v == u]
        assert len(mine) == max(1, len(items) - (L + T) + 1)
        whole = ([I] * (L + T) + items)[-(L + T):]
        assert list(seq_list[mine[0]]) == whole[:L] and list(pos_list[mine[0]]) == whole[-T:]
    np.random.seed(int(g["epoch_seed"]))
    users, seq, pos, neg, rows = epoch_feeds(users_list, seq_list, pos_list, train, I, N, B,
                                             sampler=P.numpy_batch_randint_choice)
    assert seq.dtype == np.int32 and len(seq) == -(-len(users_list) // B)
    for got, name in ((users, "users"), (seq, "seq"), (pos, "pos"), (neg, "neg"), (rows, "rows")):
        assert np.array_equal(got, g["epoch_" + name]), name
    assert rows[-1] == len(users_list) - B * (len(seq) - 1)
    for s in range(len(seq)):
        for r in range(rows[s]):
            assert not set(neg[s, r].tolist()) & set(train[int(users[s, r])])


def test_the_restatement_runs_the_recorded_epoch_to_the_reference_s_end_tables(golden):
    """train_model()'s epoch (rate 0) holds pad targets; the reference ran it with the gather of TF on a GPU"""
    g = golden
    d, L, T, N, nv, nh, l2, _ = CASES["first"]
    I = int(g["shape"][1])
    init = case_init(g, "epoch")
    rows = g["epoch_rows"]
    feeds = [tuple(g["epoch_" + k][s][:rows[s]] for k in ("users", "seq", "pos", "neg")) for s in range(len(rows))]
    assert sum(int((f[2] == I).sum()) for f in feeds) > 0
    tabs, _ = P.train(init, feeds, I, nv, nh, 0.0, l2, None, "first", np.float64, float(g["lr"]))
    for n in P.table_names(L):
        want = golden_table(g, "epoch", n, 0, init)
        lost = 2.0 ** -24 * np.abs(g["epoch_f64_" + n][0]).max()
        assert np.abs(tabs[-1][n] - want).max() <= lost + 1e-10, n


# ------------------------------------------------------------------ the maker
def test_the_makers_shim_ops_and_the_reference_s_creation_order():
    """tests/golden/make_golden_caser.py attaches the ops Caser.py needs beyond the shim's and checks each on a
    hand-computed value; with the reference tree at hand, the class's variables come in table_names' order and shapes.
    The shim is put back as it was."""
    from oracle import ref_models as rm
    from oracle import tf_shim
    spec = importlib.util.spec_from_file_location("make_golden_caser",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_caser.py"))
    path = list(sys.path)
    before = dict(vars(tf_shim))
    nn_before, had_shape = dict(vars(tf_shim.nn)), hasattr(tf_shim.Tensor, "get_shape")
    try:
        maker = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(maker)
        maker.G.attach_ops()
        assert maker.attach_caser_ops() is True
        for k in ("Conv2D", "Dense", "Dropout"):
            assert hasattr(tf_shim.layers, k), k
        assert hasattr(tf_shim, "reduce_max") and hasattr(tf_shim, "initializers")
        if rm.available():
            from make_golden_tfgraph import toy_matrix
            R = toy_matrix(isolated=False)
            ds = maker.TimedDataset(R, maker.time_orders(R))
            model, _ = maker.build(ds, maker._hyper("fourth", 20), "float64")
            d, L, T, N, nv, nh, _, _ = CASES["fourth"]
            shapes = [tuple(v.value.shape) for v in tf_shim._GRAPH.variables]
            want = [(157, d), (131, d), (131, 2 * d), (131,), (L, 1, 1, nv), (nv,)]
            for i in range(1, L + 1):
                want += [(i, d, 1, nh), (nh,)]
            want += [(nv * d + nh * L, d), (d,)]
            assert shapes == want and len(want) == len(P.table_names(L))
    finally:
        for k in list(vars(tf_shim)):
            if k not in before:
                delattr(tf_shim, k)
        for k, v in before.items():
            setattr(tf_shim, k, v)
        for k in list(vars(tf_shim.nn)):
            if k not in nn_before:
                delattr(tf_shim.nn, k)
        for k, v in nn_before.items():
            setattr(tf_shim.nn, k, v)
        if not had_shape and hasattr(tf_shim.Tensor, "get_shape"):
            del tf_shim.Tensor.get_shape
        tf_shim._GRAPH.__dict__.pop("collections", None)
        tf_shim.set_float("float32")
        tf_shim.reset_default_graph()
        sys.path[:] = path


# ------------------------------------------------------------------ the plugin and the engine on the host
def test_find_recommender_resolves_caser():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import SeqAbstractRecommender
    cls = find_recommender("Caser")
    assert cls.__module__ == "neurec_amd.model.sequential_recommender.Caser" and issubclass(cls, SeqAbstractRecommender)
    assert "Deviations" in sys.modules[cls.__module__].__doc__


def test_the_defaults_row_equals_the_reference_s_properties_file(tmp_path):
    """defaults.MODELS["Caser"] against the copy of the reference's conf/Caser.properties under tests/golden/"""
    from neurec_amd import defaults
    ref = configparser.ConfigParser()
    ref.optionxform = str
    assert ref.read(os.path.join(GOLDEN, "neurec_conf", "conf", "Caser.properties"))
    want = dict(ref["hyperparameters"])
    assert list(want) == ["lr", "l2_reg", "factors_num", "seq_L", "seq_T", "nv", "nh", "dropout", "neg_samples",
                          "batch_size", "epochs"]
    assert dict(defaults.MODELS["Caser"]) == want and [k for k, _ in defaults.MODELS["Caser"]] == list(want)
    path = defaults.write_default_configs(str(tmp_path))
    from neurec_amd.util.configurator import Configurator
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=Caser"])
    finally:
        os.chdir(cwd)
    assert (conf["factors_num"], conf["seq_L"], conf["seq_T"], conf["nv"], conf["nh"]) == (50, 5, 3, 4, 16)
    assert (conf["lr"], conf["l2_reg"], conf["dropout"], conf["neg_samples"], conf["batch_size"]) == \
        (0.001, 0.001, 0.5, 3, 256)


def test_the_plugin_refuses_a_multi_rank_run_by_name(monkeypatch):
    from neurec_amd import parallel
    from neurec_amd.model.sequential_recommender.Caser import Caser
    model = Caser.__new__(Caser)
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)
    with pytest.raises(NotImplementedError, match="Caser runs on one GPU"):
        model.build_graph()


def _make_engine(d=4, L=3, T=2, N=2, nv=2, nh=2, max_batch=8, rate=0.0):
    from neurec_amd.caser import CaserEngine
    tab = P.init_tables(5, 7, d, L, nv, nh, seed=1)
    return CaserEngine(tab, 0.001, 0.0, max_batch, T, N, nv, nh, rate)


def test_the_engine_refuses_shapes_by_name():
    """refused before a device is asked for"""
    for kw, text in ((dict(d=129), r"factors_num=129 is not supported \(1 to 128\)"),
                     (dict(L=11), r"seq_L=11 is not supported \(1 to 10\)"),
                     (dict(nv=17), r"nv=17 is not supported \(1 to 16\)"),
                     (dict(nh=65), r"nh=65 is not supported \(1 to 64\)"),
                     (dict(T=17), r"seq_T=17 is not supported \(1 to 16\)"),
                     (dict(N=0), r"neg_samples=0 is not supported \(1 to 16\)"),
                     (dict(max_batch=4097), r"max_batch=4097 is not supported \(1 to 4096\)")):
        with pytest.raises(NotImplementedError, match=text):
            _make_engine(**kw)
    with pytest.raises(ValueError, match="dropout"):
        _make_engine(rate=1.0)


def test_the_creation_order_of_the_engine_s_tables():
    from neurec_amd import caser
    assert caser.table_names(3) == P.table_names(3) == [
        "user_embeddings", "seq_item_embeddings", "item_embeddings", "item_biases", "conv_v_kernel", "conv_v_bias",
        "conv_h1_kernel", "conv_h1_bias", "conv_h2_kernel", "conv_h2_bias", "conv_h3_kernel", "conv_h3_bias",
        "fc1_kernel", "fc1_bias"]
    assert caser.SPARSE_FORM == P.SPARSE_FORM == ("user_embeddings", "item_embeddings", "item_biases")


def test_the_header_declares_the_entries_and_lib_binds_them():
    from neurec_amd import _lib, build, caser
    with open(os.path.join(ROOT, "include", "neurec_hip.h")) as f:
        text = f.read()
    for name in ("nrhip_caser_step", "nrhip_caser_forward", "nrhip_caser_workspace_floats", "nrhip_caser_scores"):
        assert re.search(r"^int %s\(" % name, text, re.M) and name in _lib.SIGNATURES, name
        above = re.findall(r"^/\*.*?\*/", text[:text.index("int %s(" % name)], re.S | re.M)[-1]
        assert re.search(r"[Rr]eplaces", above), name
    assert re.search(r"#define NRHIP_ABI_VERSION 4\b", text)
    for macro, value in (("MAX_WIDTH", caser.MAX_WIDTH), ("MAX_LEN", caser.MAX_LEN), ("MAX_NV", caser.MAX_NV),
                         ("MAX_NH", caser.MAX_NH), ("MAX_TARGETS", caser.MAX_TARGETS), ("MAX_BATCH", caser.MAX_BATCH)):
        assert re.search(r"#define NRHIP_CASER_%s %d\b" % (macro, value), text), macro
    assert _lib.CASER_MAX_LEN == caser.MAX_LEN
    for struct, cls, tail in (("nrhip_caser_weights", _lib.CaserWeights, ["n_users", "n_items", "d", "L", "nv", "nh"]),
                              ("nrhip_caser_step_args", _lib.CaserStepArgs, ["batch", "T", "N", "step", "rate", "l2_reg"])):
        block = text[text.index("typedef struct %s {" % struct):text.index("} %s;" % struct)]
        names = re.findall(r"(?:\*\s*d_|\bnrhip_caser_weights |uint64_t )(\w+)(?:\[\w+\])*;", block)
        fields = [n for n, _ in cls._fields_]
        assert fields[:len(names)] == names and fields[len(names):] == tail, struct
    assert "caser.hip" in build.SOURCES


def test_the_c_entries_refuse_by_name():
    """the bounds of the C entries (host code of the library: no GPU needed, nothing is launched)"""
    from neurec_amd import _lib
    floats = C.c_size_t(0)
    for args, text in (((8, 3, 129, 2, 2, 1, 1), r"factors_num 129 outside 1\.\.128"),
                       ((8, 11, 4, 2, 2, 1, 1), r"seq_L 11 outside 1\.\.10"),
                       ((8, 3, 4, 17, 2, 1, 1), r"nv 17 outside 1\.\.16"), ((8, 3, 4, 2, 65, 1, 1), r"nh 65 outside 1\.\.64"),
                       ((8, 3, 4, 2, 2, 17, 1), r"seq_T 17 outside 1\.\.16"),
                       ((8, 3, 4, 2, 2, 1, 0), r"neg_samples 0 outside 1\.\.16"),
                       ((4097, 3, 4, 2, 2, 1, 1), r"batch 4097 outside 0\.\.4096")):
        with pytest.raises(NotImplementedError, match=text):
            _lib.call("nrhip_caser_workspace_floats", *args, C.byref(floats))
    _lib.call("nrhip_caser_workspace_floats", 8, 3, 4, 2, 2, 2, 3, C.byref(floats))
    F = 2 * 4 + 2 * 3
    assert floats.value >= 8 * (2 * 3 * 4 + 2 * F + 3 * 2 + 4 * 4 + 2 * 5)
    a = _lib.CaserStepArgs()
    a.w.d, a.w.L, a.w.nv, a.w.nh, a.T, a.N, a.batch = 4, 3, 2, 2, 1, 1, 4097
    with pytest.raises(NotImplementedError, match=r"batch 4097 outside 0\.\.4096"):
        _lib.call("nrhip_caser_step", C.byref(a), None)
    a.batch = 2
    with pytest.raises(ValueError, match="null weight pointer"):
        _lib.call("nrhip_caser_step", C.byref(a), None)
    w = _lib.CaserWeights()
    w.d, w.L, w.nv, w.nh = 4, 11, 2, 2
    with pytest.raises(NotImplementedError, match="seq_L 11 outside"):
        _lib.call("nrhip_caser_forward", C.byref(w), None, None, 2, None, None, 8, None)
    with pytest.raises(NotImplementedError, match=r"caser_scores: width 257 outside 1\.\.256"):
        _lib.call("nrhip_caser_scores", None, 257, None, 2, 3, 257, None, 3, None)
