"""NeuMF and MLP without a GPU: the float64 restatement (tests/neumf_restatement.py) against the trace the reference's own
classes left in tests/golden/tfgraph_neumf.npz, its gradients against central differences, the split of the first layer,
the plugins' refusals, the pretrain loader, the settings files and the C entries' refusals."""
import configparser
import inspect
import os
import pickle
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import neumf_restatement as P
from neumf_restatement import CASES


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_neumf")


def case_init(g, case):
    """the seeded initial variables of a case (`epoch`: the recorded epoch's, the shape of EPOCH_CASE)"""
    U, I = (int(x) for x in g["shape"])
    _, layers, d = CASES[P.EPOCH_CASE if case == "epoch" else case][:3]
    return P.init_tables(U, I, d, layers, int(g["%s_init_seed" % case]))


def golden_table(g, case, name, step, init):
    """variable `name` after step `step` (0-based) of the float64 trace, and the storage's own rounding bound"""
    i64 = init[name].astype(np.float64)
    if "%s_q_%s" % (case, name) in g:
        scale = float(g["%s_scale_%s" % (case, name)][step])
        return i64 + g["%s_q_%s" % (case, name)][step].astype(np.float64) * scale, 0.5 * scale
    delta = g["%s_f64_%s" % (case, name)][step].astype(np.float64)
    return i64 + delta, 2.0 ** -24 * np.abs(delta).max(initial=0)


def case_feeds(g, case):
    return list(zip(g[case + "_users"], g[case + "_items"], g[case + "_labels"]))


def test_the_cases_cover_the_issue_s_list(golden):
    assert sorted(CASES) == sorted(str(c) for c in golden["cases"])
    assert CASES["default"][1:5] == ([64, 32, 16], 16, "cross_entropy", "adam")
    assert CASES["odd"][1][0] % 2 == 1 and CASES["one"][1] == [10] and CASES["wide"][1:3] == ([128, 64], 64)
    assert CASES["mlp"][0] == "MLP" and CASES["mlp"][2] == 0
    for case, row in CASES.items():
        users, items, labels = golden[case + "_users"], golden[case + "_items"], golden[case + "_labels"]
        assert users.shape == (row[7], 20) == items.shape == labels.shape
        assert row[7] == (2 if case in ("gd", "adagrad", "rmsprop", "momentum") else 4)
        for u, i, y in zip(users, items, labels):                       # the three kinds of repeat in every batch
            inst = list(zip(u.tolist(), i.tolist(), y.tolist()))
            assert len(set(inst)) < 20 and len(set(u.tolist())) < 19 and len(set(i.tolist())) < 19
            assert set(y.tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_restatement_equals_the_f64_trace(golden, case):
    """each step's loss and every variable after every step; the margin is float64's, plus what the golden's storage
    rounds away (half a count of the int16 packing, 2^-24 of a float32 difference)"""
    g = golden
    _, layers, d, loss, learner, reg_mf, reg_mlp, steps = CASES[case]
    init = case_init(g, case)
    st = P.State(init, layers, learner, float(g["lr"]))
    for s, (users, items, labels) in enumerate(case_feeds(g, case)):
        term, reg = st.step(users, items, labels, loss, reg_mf, reg_mlp)
        want = float(g[case + "_loss_f64"][s])
        assert abs(term + reg - want) <= 1e-12 * max(abs(want), 1.0), (case, s)
        for name in P.names(layers, d):
            ref, stored = golden_table(g, case, name, s, init)
            err = np.abs(st.var[name] - ref).max(initial=0)
            assert err <= stored + 1e-12 * max(np.abs(ref).max(initial=0), 1.0), (case, s, name, err, stored)
    # the learner moved every kind of variable
    assert all(np.abs(st.var[n] - init[n]).max(initial=0) > 0 for n in P.names(layers, d) if init[n].size)


def test_the_restatement_runs_the_recorded_epoch_to_the_reference_s_end_tables(golden):
    g = golden
    _, layers, d, loss, learner, reg_mf, reg_mlp, _ = CASES[P.EPOCH_CASE]
    init = case_init(g, "epoch")
    st = P.State(init, layers, learner, float(g["lr"]))
    rows = g["epoch_rows"]
    assert (rows[:-1] == int(g["batch_epoch"])).all() and 1 <= rows[-1] <= int(g["batch_epoch"])
    nnz = len(g["indices"])
    assert rows.sum() == 5 * nnz                                   # every train pair once, and num_neg = 4 negatives
    for s, n in enumerate(rows):
        st.step(g["epoch_users"][s, :n], g["epoch_items"][s, :n], g["epoch_labels"][s, :n], loss, reg_mf, reg_mlp)
    for name in P.names(layers, d):
        ref, stored = golden_table(g, "epoch", name, 0, init)
        err = np.abs(st.var[name] - ref).max()
        assert err <= stored + 1e-10 * np.abs(ref).max(), (name, err, stored)


@pytest.mark.parametrize("case", P.PREDICT_CASES)
def test_the_restatement_s_scores_equal_predict_in_both_modes(golden, case):
    g = golden
    _, layers, d, loss, learner, reg_mf, reg_mlp, _ = CASES[case]
    st = P.State(case_init(g, case), layers, learner, float(g["lr"]))
    for users, items, labels in case_feeds(g, case):
        st.step(users, items, labels, loss, reg_mf, reg_mlp)
    users, cand = g["predict_users"], g["predict_cand"]
    assert len(users) == 27 and cand.shape == (27, 3)
    want = g["predict_%s_f64" % case]
    assert want.shape == (27, 131)
    got = P.scores(st.var, users, layers)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    want_c = g["predict_cand_%s_f64" % case]
    got_c = np.stack([P.forward(st.var, np.full(3, u), c, layers)[0] for u, c in zip(users, cand)])
    assert np.abs(got_c - want_c).max() <= 1e-12 * np.abs(want_c).max()
    assert np.array_equal(got_c, np.stack([got[k][c] for k, c in enumerate(cand)]))


@pytest.mark.parametrize("layers,d,loss", [([7, 5, 3], 3, "square"), ([6, 4], 0, "cross_entropy"),
                                           ([10], 5, "cross_entropy"), ([33, 17, 9, 5], 17, "square")])
def test_the_gradients_equal_central_differences(layers, d, loss):
    """at a point with no pre-activation near 0 (checked): the loss is smooth there, so central differences of step h
    are off by O(h^2)"""
    U, I, B, h = 9, 11, 12, 1e-5
    rs = np.random.RandomState(32)
    users, items = rs.randint(0, U, B), rs.randint(0, I, B)
    users[3], items[5] = users[0], items[1]
    users[7], items[7] = users[2], items[2]
    labels = rs.randint(0, 2, B).astype(np.float64)
    labels[7] = labels[2]
    for seed in range(31, 131):                           # the first seeded point that keeps its distance from every kink
        tab = {k: v.astype(np.float64) for k, v in P.init_tables(U, I, d, layers, seed=seed).items()}
        _, _, pre = P.forward(tab, users, items, layers)
        if min(np.abs(z).min() for z in pre) > 100 * h:
            break
    assert min(np.abs(z).min() for z in pre) > 100 * h
    assert any((z < 0).any() for z in pre) and any((z > 0).any() for z in pre)
    (term, reg), G = P.gradients(tab, users, items, labels, layers, loss, 0.03, 0.05)
    assert abs(term + reg - P.total_loss(tab, users, items, labels, layers, loss, 0.03, 0.05)) < 1e-12
    for name, grad in G.items():
        flat = tab[name].reshape(-1)
        picks = rs.choice(flat.size, min(flat.size, 12), replace=False) if flat.size else []
        for k in picks:
            keep = flat[k]
            flat[k] = keep + h
            up = P.total_loss(tab, users, items, labels, layers, loss, 0.03, 0.05)
            flat[k] = keep - h
            down = P.total_loss(tab, users, items, labels, layers, loss, 0.03, 0.05)
            flat[k] = keep
            want = (up - down) / (2 * h)
            assert abs(grad.reshape(-1)[k] - want) <= 1e-6 * max(abs(want), 1.0), (name, k, grad.reshape(-1)[k], want)


def zero_pre_activation_point():
    """(tables, layers, batch): the second layer's kernel and bias are zero, so its pre-activations are exactly 0"""
    U, I, layers, d = 9, 11, [6, 4, 3], 2
    tab = P.init_tables(U, I, d, layers, seed=41)
    tab["kernel1"][:] = 0.0
    tab["bias1"][:] = 0.0
    rs = np.random.RandomState(42)
    return tab, layers, (rs.randint(0, U, 10).astype(np.int32), rs.randint(0, I, 10).astype(np.int32),
                         rs.randint(0, 2, 10).astype(np.float32))


def test_relu_passes_nothing_at_a_pre_activation_of_exactly_zero():
    """relu's gradient is 0 where the pre-activation is <= 0, the zero included (TF's ReluGrad tests `> 0`)"""
    tab, layers, (users, items, labels) = zero_pre_activation_point()
    _, _, pre = P.forward(tab, users, items, layers)
    assert not pre[1].any()
    _, G = P.gradients(tab, users, items, labels, layers, "square")
    assert not G["kernel1"].any() and not G["bias1"].any() and not G["kernel0"].any()
    assert not G["mlp_embedding_user"].any() and G["bias2"].any() and G["mf_embedding_user"].any()


@pytest.mark.parametrize("layers,d", [([64, 32, 16], 16), ([7, 5, 3], 3), ([10], 5), ([1], 2), ([8, 4], 0)])
def test_the_split_first_layer_equals_the_unsplit_one(layers, d):
    """relu((m | n) W1 + b1) = relu((m W1u + b1) + n W1i): the device scorer's form"""
    U, I = 13, 37
    tab = P.init_tables(U, I, d, layers, seed=5)
    users = np.asarray([0, 12, 5, 5])
    want = P.scores(tab, users, layers)
    got = P.scores_split(tab, users, layers)
    assert want.shape == got.shape == (4, I) and np.abs(got - want).max() <= 1e-13 * max(np.abs(want).max(), 1.0)


# ------------------------------------------------------------------ the plugins
def _plugin(name, **attrs):
    from neurec_amd.main import find_recommender
    cls = find_recommender(name)
    model = cls.__new__(cls)
    base = dict(is_pairwise=False, layers=[64, 32, 16], embedding_size=16)
    base.update(attrs)
    for k, v in base.items():
        setattr(model, k, v)
    return model


def test_find_recommender_resolves_both():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import AbstractRecommender
    for name in ("NeuMF", "MLP"):
        cls = find_recommender(name)
        assert cls.__module__ == "neurec_amd.model.general_recommender." + name and issubclass(cls, AbstractRecommender)
        assert "Deviations" in sys.modules[cls.__module__].__doc__
        assert not hasattr(cls, "get_eval_factors")                # not a factor model
        assert list(inspect.signature(cls.__init__).parameters) == ["self", "sess", "dataset", "conf"]


def test_the_plugins_read_the_reference_s_config_keys():
    from neurec_amd.model.general_recommender import MLP as mlp, NeuMF as neumf
    keys = re.findall(r'conf\["(\w+)"\]', inspect.getsource(neumf.NeuMF.__init__))
    assert keys == ["embedding_size", "layers", "reg_mf", "reg_mlp", "learning_rate", "learner", "loss_function",
                    "epochs", "num_neg", "batch_size", "verbose", "is_pairwise", "mf_pretrain", "mlp_pretrain",
                    "init_method", "stddev"]
    keys = re.findall(r'conf\["(\w+)"\]', inspect.getsource(mlp.MLP.__init__))
    assert sorted(keys) == sorted(["layers", "learning_rate", "is_pairwise", "learner", "epochs", "num_neg", "reg_mlp",
                                   "batch_size", "loss_function", "verbose", "init_method", "stddev"])


def test_pairwise_mode_is_refused_with_the_reason():
    with pytest.raises(NotImplementedError, match="second, unshared layer stack"):
        _plugin("NeuMF", is_pairwise=True).build_graph()
    with pytest.raises(NotImplementedError, match="is_pairwise=True is not supported"):
        _plugin("MLP", is_pairwise=True).build_graph()


@pytest.mark.parametrize("name", ["NeuMF", "MLP"])
def test_shapes_outside_the_kernels_are_refused_by_name(name):
    for attrs, text in ((dict(layers=[64, 32, 16, 8, 4]), r"is not supported \(1 to 4 layers\)"),
                        (dict(layers=[]), r"is not supported \(1 to 4 layers\)"),
                        (dict(layers=[129, 8]), r"layers\[0\]=129 is not supported \(1 to 128\)"),
                        (dict(layers=[64, 0]), r"layers\[1\]=0 is not supported \(1 to 128\)")):
        with pytest.raises(NotImplementedError, match=text):
            _plugin(name, **attrs).build_graph()
    if name == "NeuMF":
        for d in (129, 0):
            with pytest.raises(NotImplementedError, match=r"embedding_size=%d is not supported" % d):
                _plugin(name, embedding_size=d).build_graph()


def test_the_plugins_refuse_a_multi_rank_run_by_name(monkeypatch):
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)
    for name in ("NeuMF", "MLP"):
        with pytest.raises(NotImplementedError, match=name + " runs on one GPU"):
            _plugin(name).build_graph()


def test_the_pretrain_pickles_round_trip_through_the_loader(tmp_path):
    """both files as [user_table, item_table]; one missing, or one that is no pickle, gives None (the fallback)"""
    from neurec_amd.model.general_recommender.NeuMF import initial_variables, load_pretrained
    rs = np.random.RandomState(3)
    mf = [rs.randn(7, 4).astype(np.float32), rs.randn(9, 4).astype(np.float32)]
    mlp = [rs.randn(7, 3).astype(np.float32), rs.randn(9, 3).astype(np.float32)]
    a, b = str(tmp_path / "GMF"), str(tmp_path / "MLP")
    with open(a, "wb") as f:
        pickle.dump(mf, f)
    assert load_pretrained(a, b) is None                         # the second file is missing
    with open(b, "wb") as f:
        pickle.dump(mlp, f)
    params = load_pretrained(a, b)
    assert all(np.array_equal(x, y) for x, y in zip(params[0] + params[1], mf + mlp))
    V = initial_variables(7, 9, 4, [6, 2], "normal", 0.01, params)
    assert list(V) == P.names([6, 2], 4)
    assert all(np.array_equal(V[n], t) for n, t in zip(P.TABLES, mf + mlp))
    assert V["kernel0"].shape == (6, 6) and V["kernel1"].shape == (6, 2) and not V["bias0"].any()    # always fresh
    with open(b, "wb") as f:
        f.write(b"not a pickle")
    assert load_pretrained(a, b) is None
    assert load_pretrained("pretrain/GMF", "pretrain/MLP") is None


def test_the_initial_values():
    """creation order, shapes, the initializer's scale, glorot-uniform kernels, zero biases; the same on every call;
    an odd layers[0] gives the first kernel 2 * (layers[0] // 2) rows"""
    from neurec_amd.model.general_recommender.NeuMF import initial_variables
    V = initial_variables(50, 40, 16, [7, 5], "normal", 0.01)
    assert list(V) == P.names([7, 5], 16)
    assert {k: v.shape for k, v in V.items()} == P.shapes(50, 40, 16, [7, 5]) and V["kernel0"].shape == (6, 7)
    for n in P.TABLES:
        assert V[n].dtype == np.float32 and 0.005 < V[n].std() < 0.02
    lim = np.sqrt(6.0 / 13)
    assert 0.7 * lim < np.abs(V["kernel0"]).max() <= lim and not V["bias0"].any() and not V["bias1"].any()
    again = initial_variables(50, 40, 16, [7, 5], "normal", 0.01)
    assert all(np.array_equal(V[k], again[k]) for k in V)
    M = initial_variables(50, 40, 0, [8, 4], "normal", 0.01, with_mf=False)
    assert list(M) == P.names([8, 4], 0) and "mf_embedding_user" not in M


def test_the_settings_files_parse_to_the_reference_s_values(tmp_path):
    """defaults.MODELS against the copies of the reference's conf/NeuMF.properties and conf/MLP.properties"""
    from neurec_amd import defaults
    from neurec_amd.util.configurator import Configurator
    for name in ("NeuMF", "MLP"):
        ref = configparser.ConfigParser()
        ref.optionxform = str
        assert ref.read(os.path.join(GOLDEN, "neurec_conf", "conf", name + ".properties"))
        want = dict(ref["hyperparameters"])
        assert dict(defaults.MODELS[name]) == want and [k for k, _ in defaults.MODELS[name]] == list(want)
    path = defaults.write_default_configs(str(tmp_path))
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=NeuMF"])
        mlp = Configurator(path, default_section="hyperparameters", argv=["--recommender=MLP"])
    finally:
        os.chdir(cwd)
    assert (conf["epochs"], conf["batch_size"], conf["embedding_size"], conf["layers"]) == (100, 256, 16, [64, 32, 16])
    assert (conf["reg_mf"], conf["reg_mlp"], conf["is_pairwise"], conf["num_neg"]) == (0, 0, False, 4)
    assert (conf["loss_function"], conf["learning_rate"], conf["learner"]) == ("cross_entropy", 0.001, "adam")
    assert (conf["init_method"], conf["stddev"], conf["verbose"]) == ("normal", 0.01, 1)
    assert (conf["mf_pretrain"], conf["mlp_pretrain"]) == ("pretrain/GMF", "pretrain/MLP")
    assert (mlp["layers"], mlp["reg_mlp"], mlp["is_pairwise"], mlp["loss_function"]) == ([64, 32, 16], 0.0, True, "bpr")


# ------------------------------------------------------------------ the C boundary
def test_the_header_declares_the_entries_and_lib_binds_them():
    from neurec_amd import _lib, neumf
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "neurec_hip.h")) as f:
        text = f.read()
    for sym in ("nrhip_neumf_workspace_floats", "nrhip_neumf_step", "nrhip_neumf_forward",
                "nrhip_neumf_scores_workspace_floats", "nrhip_neumf_scores"):
        assert re.search(r"\b%s\s*\(" % sym, text) and sym in _lib.SIGNATURES
    for macro, value in (("NRHIP_NEUMF_MAX_WIDTH", neumf.MAX_WIDTH), ("NRHIP_NEUMF_MAX_LAYERS", neumf.MAX_LAYERS),
                         ("NRHIP_NEUMF_MAX_BATCH", neumf.MAX_BATCH)):
        assert "#define %s %d" % (macro, value) in text
    assert _lib.NEUMF_MAX_LAYERS == neumf.MAX_LAYERS
    # the two structs as a C compiler lays them out: pointers, then ints / floats, no holes but the tail's
    import ctypes as C
    assert C.sizeof(_lib.NeumfWeights) == 12 * 8 + 8 * 4
    assert C.sizeof(_lib.NeumfStepArgs) == C.sizeof(_lib.NeumfWeights) + 22 * 8 + 4 * 4


def test_the_c_entries_refuse_by_name():
    import ctypes as C
    from neurec_amd import _lib
    n = C.c_size_t(0)

    def weights(d, layers):
        w = _lib.NeumfWeights()
        w.n_users, w.n_items, w.d, w.n_layers = 5, 7, d, len(layers)
        for k, x in enumerate(layers[:4]):
            w.width[k] = x
        return w
    _lib.call("nrhip_neumf_workspace_floats", C.byref(weights(16, [64, 32, 16])), 256, C.byref(n))
    assert n.value >= 32 * (64 * 64 + 64 + 64 * 32 + 32 + 32 * 16 + 16)
    for d, layers, batch, text in ((129, [8], 4, r"embedding_size 129 outside 0\.\.128"),
                                   (4, [8, 129], 4, r"layers\[1\] = 129 outside 1\.\.128"),
                                   (4, [0], 4, r"layers\[0\] = 0 outside 1\.\.128"),
                                   (4, [8] * 5, 4, r"5 layers outside 1\.\.4"),
                                   (4, [8], 4097, r"batch 4097 outside 0\.\.4096")):
        with pytest.raises(NotImplementedError, match=text):
            _lib.call("nrhip_neumf_workspace_floats", C.byref(weights(d, layers)), batch, C.byref(n))
    a = _lib.NeumfStepArgs()
    a.w = weights(4, [8, 4])
    a.batch, a.loss_kind = 3, 7
    with pytest.raises(ValueError, match="unknown pointwise loss 7"):
        _lib.call("nrhip_neumf_step", C.byref(a), None)
    a.loss_kind = 0
    with pytest.raises(ValueError, match="null"):
        _lib.call("nrhip_neumf_step", C.byref(a), None)
    a.batch = 0                                                    # an empty batch is no work, whatever the pointers
    _lib.call("nrhip_neumf_step", C.byref(a), None)
