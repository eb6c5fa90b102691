"""SASRec without a GPU: the numpy restatement (tests/sasrec_restatement.py) against the trace of the reference class in
both of its forms, the suffix form against the full-mask form on awkward rows, the plugin's feeds against the recorded
epoch, the creation order, the refusals and defaults, the maker's attached shim ops and the C entries' bounds."""
import configparser
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from conftest import load_golden
import sasrec_restatement as P
from sasrec_restatement import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_sasrec")


def case_inputs(g, case):
    d, h, nb, L, l2, rate = CASES[case]
    names = P.table_names(nb)
    init = {n: g["%s_init_%s" % (case, n)] for n in names}
    S = len(g[case + "_seq"])
    feeds = [(g[case + "_seq"][s], g[case + "_pos"][s], g[case + "_neg"][s]) for s in range(S)]
    masks = [[g["%s_mask%d" % (case, k)][s] for k in range(P.n_sites(nb))] for s in range(S)] if rate else None
    return names, init, feeds, masks


def golden_table(g, case, tag, name, s):
    """the whole variable after step s + 1 of the trace in float64: initial value + stored difference"""
    t = g["%s_init_%s" % (case, name)].astype(np.float64)
    delta = g["%s_%s_%s" % (case, tag, name)][s].astype(np.float64)
    if name == "item_emb":
        t[g["%s_rows_item_emb" % case]] += delta
    else:
        t += delta
    return t


def test_the_cases_cover_the_issue_s_list(golden):
    g = golden
    assert CASES == {"first": (12, 1, 2, 7, 0.0, 0.0), "second": (8, 2, 1, 5, 0.01, 0.5), "third": (50, 1, 2, 10, 0.0, 0.5)}
    assert sorted(g["cases"].tolist()) == sorted(CASES) and tuple(g["shape"]) == (157, 131) and int(g["batch_step"]) == 20
    I = int(g["shape"][1])
    lens = np.diff(g["seq_ptr"])
    for case, (d, h, nb, L, l2, rate) in CASES.items():
        seq, pos, neg = g[case + "_seq"], g[case + "_pos"], g[case + "_neg"]
        assert seq.shape == (3, 20, L) and pos.shape == seq.shape and neg.shape == seq.shape
        n_real = (seq != I).sum(2)
        for s in range(3):                       # every kind of row in every step
            assert (n_real[s] == 0).any() and (n_real[s] == 1).any() and (n_real[s] == L).any()
            assert ((n_real[s] > 1) & (n_real[s] < L)).any()
        assert ((pos != I) == (seq != I)).all() and ((neg != I) == (seq != I)).all()
        real = seq != I                          # pre-padding: the real positions are a suffix
        assert (real[:, :, 1:] >= real[:, :, :-1]).all()
        assert (lens - 1 > L).any() and (lens - 1 == L).any() and (lens == 1).any()
        if rate:
            shapes = P.site_shapes(20, L, d, h, nb)
            for k, shp in enumerate(shapes):
                m = g["%s_mask%d" % (case, k)]
                assert m.shape == (3,) + shp and m.dtype == np.uint8 and set(np.unique(m)) == {0, 1}
        else:
            assert case + "_mask0" not in g


@pytest.mark.parametrize("form", ["mask", "suffix"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_restatement_equals_the_f64_trace(golden, case, form):
    """losses and every variable after every step, in float64, in both forms.  The stored differences are float32
    (2^-24 of ~3e-3 lost).  Beyond that 1e-11: bk's gradient is zero in exact arithmetic (a softmax ignores a shift of
    its row), so it is float64 rounding noise of ~1e-16, which Adam's lr / eps = 1e5 lifts to 1e-11 per step."""
    g = golden
    d, h, nb, L, l2, rate = CASES[case]
    names, init, feeds, masks = case_inputs(g, case)
    tabs, losses = P.train(init, feeds, int(g["shape"][1]), h, rate, l2, masks, form, np.float64)
    assert np.abs(np.asarray(losses) - g[case + "_loss_f64"]).max() < 1e-12
    for s in range(len(feeds)):
        for n in names:
            want = golden_table(g, case, "f64", n, s)
            lost = 2.0 ** -24 * np.abs(g["%s_f64_%s" % (case, n)][s]).max()
            assert np.abs(tabs[s][n] - want).max() <= lost + 1e-11, (case, form, s, n)
    # rows of item_emb outside <case>_rows_item_emb never moved
    still = np.setdiff1d(np.arange(len(init["item_emb"])), g[case + "_rows_item_emb"])
    assert np.array_equal(tabs[-1]["item_emb"][still], init["item_emb"][still].astype(np.float64))


def test_the_float32_restatement_stays_within_the_rule_of_the_trace(golden):
    """the rule the GPU tests use, on the restatement in float32: 4x the reference's own f32-to-f64 distance plus
    1e-5 max|want|"""
    g = golden
    case = "second"
    d, h, nb, L, l2, rate = CASES[case]
    names, init, feeds, masks = case_inputs(g, case)
    tabs, _ = P.train(init, feeds, int(g["shape"][1]), h, rate, l2, masks, "suffix", np.float32)
    for s in range(len(feeds)):
        for n in names:
            w64, w32 = golden_table(g, case, "f64", n, s), golden_table(g, case, "f32", n, s)
            tol = 4 * np.abs(w32 - w64).max() + 1e-5 * np.abs(w64).max()
            assert np.abs(tabs[s][n] - w64).max() <= tol, (s, n)


def awkward_batch(I, L, d, h, nb, B, seed, beta_zero=False):
    """rows of every kind, repeated items, the same item as positive and negative, and dropout masks that drop a whole
    real row at the embedding (a zero key; with beta == 0 also a zero query) — once at a row's first real position, so
    that this query sees no key at all"""
    rs = np.random.RandomState(seed)
    T = P.init_tables(I, d, L, nb, seed)
    if beta_zero:
        for k in T:
            if k.endswith("ln1_beta"):
                T[k] = np.zeros_like(T[k])
    seq, pos, neg = (np.full((B, L), I, np.int32) for _ in range(3))
    lens = [0, 1, L, L] + rs.randint(1, L + 1, B).tolist()
    for b in range(B):
        n = min(lens[b], L)
        if n:
            seq[b, L - n:], pos[b, L - n:], neg[b, L - n:] = (rs.randint(0, I, n) for _ in range(3))
    if L > 2:
        seq[2, -1], neg[2, -2] = seq[2, -2], pos[2, -2]            # a repeated item; positive == negative
    masks = [(rs.random_sample(s) < 0.6).astype(np.uint8) for s in P.site_shapes(B, L, d, h, nb)]
    masks[0][2, 0] = 0                                             # row 2 is full: its first real position is dropped
    masks[0][1, L - 1] = 0                                         # row 1 has one item: its query sees L - 1 pads and a zero
    if L > 2:
        masks[0][3, L // 2] = 0                                    # a dropped key in the middle of row 3
    return T, seq, pos, neg, masks


@pytest.mark.parametrize("d,h,nb,L,beta_zero", [(6, 2, 2, 5, False), (6, 3, 1, 4, True), (4, 1, 3, 1, False)])
def test_the_suffix_form_equals_the_mask_form(d, h, nb, L, beta_zero):
    """The argument of DESIGN: padded rows contribute nothing, so working on each row's real suffix gives the full-mask
    form's loss and gradients.  It holds with one amendment the restatement carries: a query none of whose keys is
    visible softmaxes uniformly over all L keys, the padded ones (V = bv) and the later ones included."""
    I, B = 9, 7
    T, seq, pos, neg, masks = awkward_batch(I, L, d, h, nb, B, 5, beta_zero)
    la, Ga = P.gradients(T, seq, pos, neg, I, h, 0.4, 0.01, masks, "mask")
    lb, Gb = P.gradients(T, seq, pos, neg, I, h, 0.4, 0.01, masks, "suffix")
    assert abs(la - lb) <= 1e-13 * abs(la)
    for k in Ga:
        assert np.abs(Ga[k] - Gb[k]).max() <= 1e-12 * max(np.abs(Ga[k]).max(), 1e-3), k
    if not beta_zero and L > 2:                  # the uniform row reached bv through the padded / later keys
        assert np.abs(Ga["b0_bv"]).max() > 0
    rows = np.stack([seq[b] for b in range(B)])
    assert np.abs(P.final_rows(T, rows, I, h, "mask") - P.final_rows(T, rows, I, h, "suffix")).max() < 1e-13
    assert np.array_equal(P.final_rows(T, rows[:1], I, h)[0], T["lnf_beta"].astype(np.float64))   # the all-padded row


def test_the_gradients_equal_central_differences():
    I, B, d, h, nb, L = 7, 4, 4, 2, 1, 3
    T, seq, pos, neg, masks = awkward_batch(I, L, d, h, nb, B, 11)
    _, G = P.gradients(T, seq, pos, neg, I, h, 0.4, 0.02, masks, "mask")
    rs = np.random.RandomState(0)
    T64 = {k: v.astype(np.float64) for k, v in T.items()}
    for k in T64:
        for _ in range(3):
            idx = tuple(rs.randint(0, s) for s in T64[k].shape)
            eps = 1e-6
            up, dn = ({n: v.copy() for n, v in T64.items()} for _ in range(2))
            up[k][idx] += eps
            dn[k][idx] -= eps
            num = (P.gradients(up, seq, pos, neg, I, h, 0.4, 0.02, masks, "mask")[0] -
                   P.gradients(dn, seq, pos, neg, I, h, 0.4, 0.02, masks, "mask")[0]) / (2 * eps)
            assert abs(num - G[k][idx]) <= 1e-7 * max(1.0, abs(num)), (k, idx, num, G[k][idx])


def test_the_creation_order():
    names = P.table_names(2)
    assert names[:4] == ["item_emb", "pos_emb", "b0_ln1_beta", "b0_ln1_gamma"]          # beta before gamma
    assert names[4:10] == ["b0_Wq", "b0_bq", "b0_Wk", "b0_bk", "b0_Wv", "b0_bv"]
    assert names[10:16] == ["b0_ln2_beta", "b0_ln2_gamma", "b0_W1", "b0_b1", "b0_W2", "b0_b2"]
    assert names[16] == "b1_ln1_beta" and names[-2:] == ["lnf_beta", "lnf_gamma"] and len(names) == 2 + 2 * 14 + 2
    from neurec_amd import sasrec
    assert tuple("b0_" + n for n in sasrec.BLOCK_VARS) == tuple(names[2:16])
    assert sasrec.BETA2 == 0.98 == P.BETA2


def test_the_makers_shim_ops_and_the_reference_s_creation_order():
    """tests/golden/make_golden_sasrec.py attaches the ops SASRec.py needs beyond the shim's and checks each on a
    hand-computed value; with the reference tree at hand, the class's variables come in table_names' order and shapes.
    The shim is put back as it was."""
    from oracle import ref_models as rm
    from oracle import tf_shim
    spec = importlib.util.spec_from_file_location("make_golden_sasrec",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_sasrec.py"))
    path = list(sys.path)
    before = dict(vars(tf_shim))
    nn_before, had_shape = dict(vars(tf_shim.nn)), hasattr(tf_shim.Tensor, "get_shape")
    try:
        maker = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(maker)
        maker.G.attach_ops()
        assert maker.attach_sasrec_ops() is True
        for k in ("get_variable", "get_collection", "GraphKeys", "layers", "sign", "abs", "tile", "ones_like", "where",
                  "equal", "not_equal", "to_float", "range", "convert_to_tensor", "linalg", "variable_scope"):
            assert hasattr(tf_shim, k), k
        assert hasattr(tf_shim.nn, "moments") and hasattr(tf_shim.nn, "softmax")
        if rm.available():
            from make_golden_tfgraph import toy_matrix
            R = toy_matrix(isolated=False)
            ds = maker.TimedDataset(R, maker.time_orders(R))
            model, _ = maker.build(ds, maker._hyper("second", 20), "float64")
            d, h, nb, L, _, _ = CASES["second"]
            shapes = [tuple(v.value.shape) for v in tf_shim._GRAPH.variables]
            want = [(131, d), (L, d)] + [(d,), (d,), (d, d), (d,), (d, d), (d,), (d, d), (d,), (d,), (d,), (1, d, d), (d,),
                                         (1, d, d), (d,)] * nb + [(d,), (d,)]
            assert shapes == want
            vals = [v.numpy() for v in tf_shim._GRAPH.variables]
            assert not vals[2].any() and (vals[3] == 1).all()       # ln: beta (zeros), then gamma (ones)
            assert not vals[-2].any() and (vals[-1] == 1).all()
    finally:
        for k in list(vars(tf_shim)):
            if k not in before:
                delattr(tf_shim, k)
        for k, v in before.items():
            setattr(tf_shim, k, v)
        for k in list(vars(tf_shim.nn)):
            if k not in nn_before:
                delattr(tf_shim.nn, k)
        if not had_shape and hasattr(tf_shim.Tensor, "get_shape"):
            del tf_shim.Tensor.get_shape
        tf_shim._GRAPH.__dict__.pop("collections", None)
        tf_shim.set_float("float32")
        tf_shim.reset_default_graph()
        sys.path[:] = path


# ------------------------------------------------------------------ the feeds
def _user_dict(g):
    ptr, seq = g["seq_ptr"], g["seq"]
    return {u: seq[ptr[u]:ptr[u + 1]].tolist() for u in range(len(ptr) - 1) if ptr[u + 1] > ptr[u]}


def test_the_epoch_feeds_are_bit_equal_to_the_recorded_epoch(golden):
    """the reference's train_model() from the same seed with the same stand-in sampler on numpy's stream:
    get_train_data's draws first, then the shuffle"""
    from neurec_amd.model.sequential_recommender.SASRec import epoch_feeds, get_train_data
    g = golden
    I, B, L = int(g["shape"][1]), int(g["batch_epoch"]), CASES["first"][3]
    users = _user_dict(g)
    np.random.seed(int(g["epoch_seed"]))
    seq, pos, neg, rows = epoch_feeds(users, I, L, B, sampler=P.numpy_batch_randint_choice)
    assert seq.dtype == np.int32 and seq.shape == g["epoch_seq"].shape and len(seq) == -(-len(users) // B)
    assert np.array_equal(seq, g["epoch_seq"]) and np.array_equal(pos, g["epoch_pos"])
    assert np.array_equal(neg, g["epoch_neg"]) and np.array_equal(rows, g["epoch_rows"])
    assert rows[-1] == len(users) - B * (len(seq) - 1) and (seq[-1, rows[-1]:] == I).all()
    # the order of the stream: the sampler's draws, then one permutation
    np.random.seed(int(g["epoch_seed"]))
    s2, p2, n2 = get_train_data(users, I, L, sampler=P.numpy_batch_randint_choice)
    order = np.random.permutation(len(s2))
    assert np.array_equal(s2[order[:B]], seq[0]) and np.array_equal(n2[order[:B]], neg[0])
    # seq = items[:-1], pos = items[1:], padded and truncated in front; negatives outside the user's train items
    for r, u in enumerate(users):
        items = users[u]
        want = ([I] * L + items[:-1])[-L:]
        assert s2[r].tolist() == want and p2[r].tolist() == ([I] * L + items[1:])[-L:]
        real = n2[r][n2[r] != I]
        assert len(real) == min(len(items) - 1, L) and not set(real.tolist()) & set(items)


def test_one_and_two_item_users_are_rows():
    """the reference's sampler raises for size 0 and unwraps size 1: here an all-padded row and a one-item row"""
    from neurec_amd.model.sequential_recommender.SASRec import get_train_data
    asked = []

    def sampler(high, size, replace=True, exclusion=None):
        asked.append(list(size))
        return [7 if n == 1 else [7] * n for n in size]             # a bare int for size 1, as the reference's does
    seq, pos, neg = get_train_data({0: [3], 1: [1, 2], 2: [4, 5, 6]}, 9, 3, sampler=sampler)
    assert asked == [[1, 2]]
    assert seq.tolist() == [[9, 9, 9], [9, 9, 1], [9, 4, 5]] and pos.tolist() == [[9, 9, 9], [9, 9, 2], [9, 5, 6]]
    assert neg.tolist() == [[9, 9, 9], [9, 9, 7], [9, 7, 7]]


# ------------------------------------------------------------------ the plugin and the engine on the host
def test_find_recommender_resolves_sasrec():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import SeqAbstractRecommender
    cls = find_recommender("SASRec")
    assert cls.__module__ == "neurec_amd.model.sequential_recommender.SASRec" and issubclass(cls, SeqAbstractRecommender)
    assert "Deviations" in sys.modules[cls.__module__].__doc__


def test_defaults_are_written_for_sasrec(tmp_path):
    """defaults.MODELS["SASRec"] holds the values of the reference's conf/SASRec.properties"""
    from neurec_amd import defaults
    path = defaults.write_default_configs(str(tmp_path))
    parser = configparser.ConfigParser()
    parser.optionxform = str
    parser.read(os.path.join(str(tmp_path), "conf", "SASRec.properties"))
    want = {"lr": "0.001", "l2_emb": "0.0", "hidden_units": "50", "dropout_rate": "0.5", "max_len": "50",
            "num_blocks": "2", "num_heads": "1", "batch_size": "128", "epochs": "1000"}
    assert dict(parser["hyperparameters"]) == want
    from neurec_amd.util.configurator import Configurator
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=SASRec"])
    finally:
        os.chdir(cwd)
    assert conf["hidden_units"] == 50 and conf["max_len"] == 50 and conf["num_blocks"] == 2 and conf["num_heads"] == 1
    assert conf["batch_size"] == 128 and conf["dropout_rate"] == 0.5 and conf["l2_emb"] == 0.0 and conf["lr"] == 0.001


def test_the_plugin_refuses_by_name(monkeypatch):
    from neurec_amd import parallel
    from neurec_amd.model.sequential_recommender.SASRec import SASRec
    model = SASRec.__new__(SASRec)
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)
    with pytest.raises(NotImplementedError, match="one GPU"):
        model.build_graph()


def _make_engine(d=4, L=3, nb=1, h=1, max_batch=8, rate=0.0):
    from neurec_amd.sasrec import BLOCK_VARS, SASRecEngine
    T = P.init_tables(7, d, L, nb, seed=1)
    blocks = [[T["b%d_%s" % (i, n)] for n in BLOCK_VARS] for i in range(nb)]
    return SASRecEngine(T["item_emb"], T["pos_emb"], blocks, (T["lnf_beta"], T["lnf_gamma"]), 0.001, 0.0, max_batch, h, rate)


def test_the_engine_refuses_shapes_by_name():
    """refused before a device is asked for"""
    with pytest.raises(NotImplementedError, match=r"hidden_units=129 is not supported \(1 to 128\)"):
        _make_engine(d=129)
    with pytest.raises(NotImplementedError, match=r"max_len=201 is not supported \(1 to 200\)"):
        _make_engine(L=201)
    with pytest.raises(NotImplementedError, match=r"num_blocks=5 is not supported \(1 to 4\)"):
        _make_engine(nb=5)
    with pytest.raises(ValueError, match="num_heads=3 does not divide hidden_units=4"):
        _make_engine(h=3)
    with pytest.raises(NotImplementedError, match="max_batch=4097 is not supported"):
        _make_engine(max_batch=4097)
    with pytest.raises(NotImplementedError, match="saved attention weights"):
        _make_engine(d=128, L=200, h=128, max_batch=4096)
    with pytest.raises(ValueError, match="dropout_rate"):
        _make_engine(rate=1.0)


def test_the_header_declares_the_entries_and_lib_binds_them():
    from neurec_amd import _lib, build, sasrec
    with open(os.path.join(ROOT, "include", "neurec_hip.h")) as f:
        text = f.read()
    for name in ("nrhip_sasrec_step", "nrhip_sasrec_forward", "nrhip_sasrec_workspace_floats"):
        assert re.search(r"^int %s\(" % name, text, re.M) and name in _lib.SIGNATURES, name
        above = re.findall(r"^/\*.*?\*/", text[:text.index("int %s(" % name)], re.S | re.M)[-1]
        assert re.search(r"[Rr]eplaces", above), name
    assert re.search(r"#define NRHIP_ABI_VERSION 4\b", text)
    for macro, value in (("MAX_BLOCKS", sasrec.MAX_BLOCKS), ("MAX_WIDTH", sasrec.MAX_WIDTH), ("MAX_LEN", sasrec.MAX_LEN),
                         ("MAX_BATCH", sasrec.MAX_BATCH), ("BLOCK_VARS", len(sasrec.BLOCK_VARS))):
        assert re.search(r"#define NRHIP_SASREC_%s %d\b" % (macro, value), text), macro
    assert "#define NRHIP_SASREC_MAX_WEIGHTS (1ll << 30)" in text and sasrec.MAX_WEIGHTS == 1 << 30
    block = text[text.index("typedef struct nrhip_sasrec_step_args"):text.index("} nrhip_sasrec_step_args;")]
    names = re.findall(r"(?:\*\s*d_|\bnrhip_sasrec_weights |uint64_t )(\w+)(?:\[\w+\])*;", block)
    fields = [n for n, _ in _lib.SasrecStepArgs._fields_]
    assert fields[:len(names)] == names and fields[len(names):] == ["batch", "step", "rate", "l2_emb"]
    assert "sasrec.hip" in build.SOURCES


def test_the_c_entries_refuse_by_name():
    """the bounds of the C entries (host code of the library: no GPU needed, nothing is launched)"""
    from neurec_amd import _lib
    floats = C.c_size_t(0)
    for args, text in (((8, 3, 129, 1, 1), r"hidden_units 129 outside 1\.\.128"), ((8, 201, 4, 1, 1), r"max_len 201 outside"),
                       ((8, 3, 4, 5, 1), r"num_blocks 5 outside 1\.\.4"), ((4097, 3, 4, 1, 1), r"batch 4097 outside"),
                       ((4096, 200, 128, 1, 128), "attention weights are more than")):
        with pytest.raises(NotImplementedError, match=text):
            _lib.call("nrhip_sasrec_workspace_floats", *args, C.byref(floats))
    with pytest.raises(ValueError, match="num_heads 3 does not divide hidden_units 4"):
        _lib.call("nrhip_sasrec_workspace_floats", 8, 3, 4, 1, 3, C.byref(floats))
    _lib.call("nrhip_sasrec_workspace_floats", 8, 3, 4, 2, 2, C.byref(floats))
    assert floats.value >= 2 * (11 * 8 * 3 * 4 + 2 * 8 * 3 * 3)
    a = _lib.SasrecStepArgs()
    a.w.d, a.w.L, a.w.n_blocks, a.w.n_heads, a.batch = 4, 3, 1, 1, 4097
    with pytest.raises(NotImplementedError, match=r"batch 4097 outside 0\.\.4096"):
        _lib.call("nrhip_sasrec_step", C.byref(a), None)
    a.batch = 2
    with pytest.raises(ValueError, match="null weight pointer"):
        _lib.call("nrhip_sasrec_step", C.byref(a), None)
    w = _lib.SasrecWeights()
    w.d, w.L, w.n_blocks, w.n_heads = 4, 3, 1, 3
    with pytest.raises(ValueError, match="does not divide"):
        _lib.call("nrhip_sasrec_forward", C.byref(w), None, 2, None, 1.0, None, 4, None)
