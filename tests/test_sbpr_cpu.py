"""SBPR without a GPU: the float64 restatement the GPU tests lean on (tests/sbpr_restatement.py) against the reference
class's own social sets, suk and f64 trace; the sets against scipy's S @ R on a graph the reference cannot run; the
trust-file parsing of SocialAbstractRecommender; the C entries' declarations and refusals, the plugin's constructor, the
defaults and the dispatch of `recommender=SBPR`."""
import configparser
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_golden
import sbpr_restatement as P
from sbpr_restatement import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("users", "items", "social", "neg", "suk")


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_sbpr")


def _batch(g, case, k):
    return tuple(g["%s_%s" % (case, f)][k] for f in FIELDS)


def _sets(g):
    return P.social_sets(g["indptr"], g["indices"], g["trust_indptr"], g["trust_indices"])


def test_the_graph_and_the_cases_the_trace_was_recorded_for(golden):
    """the trust file holds users who trust nobody, users who trust themselves and duplicated lines, and no edge to a
    user without train items; some train users have an empty social set; six cases"""
    g = golden
    assert sorted(g["cases"].tolist()) == sorted(CASES) and len(CASES) == 6
    assert tuple(int(x) for x in g["shape"]) == (157, 131)
    lines = [tuple(x) for x in g["trust_lines"].tolist()]
    deg = np.diff(g["indptr"])
    assert len(set(u for u, _ in lines)) < 157 and any(u == f for u, f in lines) and len(set(lines)) < len(lines)
    assert all(deg[f] > 0 for _, f in lines)
    ptr, idx = P.trust_csr(lines, 157)
    assert np.array_equal(ptr, g["trust_indptr"]) and np.array_equal(idx, g["trust_indices"])   # duplicates collapse
    n_sets = int((np.diff(g["social_ptr"]) > 0).sum())
    assert 0 < n_sets < int((deg > 0).sum())
    assert len(g["epoch_users"]) == int(deg[np.diff(g["social_ptr"]) > 0].sum())
    for case in CASES:
        assert g[case + "_users"].shape == (P.STEPS.get(case, 2), 48) and g[case + "_suk"].dtype == np.float32
    # the duplicate case: one item as i, k and j of different slots, a user several times
    users, items, social, neg, _ = _batch(g, "bpr_adam_dup", 0)
    assert set(items) & set(social) & set(neg) and np.bincount(users).max() >= 3


def test_restatement_reproduces_the_reference_social_sets(golden):
    g = golden
    ptr, items, counts = P.sets_as_csr(_sets(g), 157)
    assert np.array_equal(ptr, g["social_ptr"]) and np.array_equal(items, g["social_items"])
    assert counts.min() >= 1


def test_restatement_suk_equals_the_recorded_suk(golden):
    """suk of every recorded (u, k) = 1 + the restatement's count; the recorded epoch obeys the instance rules"""
    g = golden
    sets = _sets(g)
    for u, k, suk in zip(g["epoch_users"], g["epoch_social"], g["epoch_suk"]):
        items, counts = sets[int(u)]
        at = np.searchsorted(items, k)
        assert items[at] == k and suk == counts[at] + 1
    want = P.eligible_positives(g["indptr"], g["indices"], sets)
    assert list(zip(g["epoch_users"].tolist(), g["epoch_items"].tolist())) == want
    for u, j in zip(g["epoch_users"], g["epoch_neg"]):
        own = g["indices"][g["indptr"][u]:g["indptr"][u + 1]]
        assert j not in own and j not in sets[int(u)][0]


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_the_f64_trace(golden, case):
    """every step of every case: the three tables and the loss within 1e-12 of the reference class's float64 run;
    predict() after the case it was recorded for, full and candidate mode"""
    g = golden
    loss, learner = CASES[case]
    st = P.State(*P.golden_tables(g, case, "f64", -1), learner=learner, lr=float(g["learning_rate"]))
    for k in range(len(g[case + "_users"])):
        got = P.step(st, *_batch(g, case, k), loss, float(g["reg_mf"]))
        want = g[case + "_f64_loss"][k]
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (k, got, want)
        for name, want in zip(P.TABLES, P.golden_tables(g, case, "f64", k)):
            err = np.abs(st.var[name] - want).max()
            assert err <= 1e-12, (case, k, name, err)
    if case == P.PREDICT_CASE:
        got = P.predict(st.var["P"], st.var["Q"], g["predict_users"])
        assert np.abs(got - g["predict_f64"]).max() <= 1e-12                 # no bias in predict()
        cand = np.stack([got[k][c] for k, c in enumerate(g["predict_cand"])])
        assert np.abs(cand - g["predict_cand_f64"]).max() <= 1e-12
        assert np.abs(st.var["b"]).max() > 0


def second_graph(g):
    """a graph the reference cannot run: edges to users without train items as well"""
    R = sp.csr_matrix((np.ones(len(g["indices"]), np.float32), g["indices"], g["indptr"]),
                      shape=tuple(int(x) for x in g["shape"]))
    lines = P.trust_graph(R, seed=77, every_empty=9, only_train_users=False)
    deg = np.diff(R.indptr)
    assert any(deg[f] == 0 for _, f in lines) and any(deg[u] == 0 for u, _ in lines)
    return R, lines, P.trust_csr(lines, R.shape[0])


def test_social_sets_equal_the_sparse_product_minus_the_own_pattern(golden):
    """on a second graph with edges to users without train items: C = pattern of (S @ R) minus R's, counts = its values"""
    R, lines, (s_ptr, s_idx) = second_graph(golden)
    U = R.shape[0]
    S = sp.csr_matrix((np.ones(len(s_idx)), s_idx, s_ptr), shape=(U, U))
    prod = (S @ R.astype(np.float64)).toarray()
    prod[R.toarray() > 0] = 0
    prod[np.diff(R.indptr) == 0] = 0                          # a user without train items is not in train_dict
    sets = P.social_sets(R.indptr, R.indices, s_ptr, s_idx)
    for u in range(U):
        want = np.flatnonzero(prod[u])
        if len(want) == 0:
            assert u not in sets
        else:
            assert np.array_equal(sets[u][0], want) and np.array_equal(sets[u][1], prod[u][want].astype(np.int32))


def test_a_user_with_no_free_item_is_refused():
    """R_u and C_u together are all the items: ValueError naming the user"""
    tr_ptr, tr_idx = np.asarray([0, 2, 4, 5], np.int64), np.asarray([0, 1, 2, 3, 0], np.int32)     # 4 items
    s_ptr, s_idx = np.asarray([0, 1, 1, 2], np.int64), np.asarray([1, 1], np.int32)               # 0 -> 1, 2 -> 1
    sets = P.social_sets(tr_ptr, tr_idx, s_ptr, s_idx)
    assert sorted(sets) == [0, 2] and sets[0][0].tolist() == [2, 3]
    with pytest.raises(ValueError, match="user 0 has no item outside"):
        P.check_no_free_item(tr_ptr, sets, 4)
    P.check_no_free_item(tr_ptr, {2: sets[2]}, 4)


# ------------------------------------------------------------------ the plugin layer
class _Dataset:
    dataset_name = "toy"

    def __init__(self, userids, n_items=5):
        self.userids = userids
        self.num_users, self.num_items = len(userids), n_items
        self.train_matrix = sp.csr_matrix((np.ones(3, np.float32), ([0, 1, 2], [0, 1, 2])),
                                          shape=(len(userids), n_items))

    def get_user_train_dict(self, by_time=False):
        return {0: [0], 1: [1], 2: [2]}

    def get_user_test_dict(self):
        return {0: [3]}

    def get_user_test_neg_dict(self):
        return None

    def __str__(self):
        return "toy dataset"


@pytest.mark.parametrize("keys", ["str", "int"])
def test_trust_file_parsing(tmp_path, keys):
    """unknown ids dropped, duplicates collapsed, the matrix directed; string and integer keys of userids both kept"""
    from neurec_amd.model.AbstractRecommender import read_trust_lines
    raw = [10, 20, 30, 40]
    userids = {(str(r) if keys == "str" else r): k for k, r in enumerate(raw)}
    path = os.path.join(str(tmp_path), "toy.uu")
    with open(path, "w") as f:
        f.write("10\t20\n10\t20\n20\t99\n98\t10\n30\t30\n40\t10\n")
    user, friend = read_trust_lines(path, "\t", userids)
    assert user.tolist() == [0, 0, 2, 3] and friend.tolist() == [1, 1, 2, 0]
    S = sp.csr_matrix(([1] * len(user), (user, friend)), shape=(4, 4))
    assert S.indices.tolist() == [1, 2, 0] and S.indptr.tolist() == [0, 1, 1, 2, 3]          # (0, 1) once; not symmetric


def test_plugin_constructor_reads_the_reference_keys(tmp_path, monkeypatch):
    from neurec_amd import defaults
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import AbstractRecommender, SocialAbstractRecommender
    cls = find_recommender("SBPR")
    assert cls.__name__ == "SBPR" and cls.__module__ == "neurec_amd.model.social_recommender.SBPR"
    assert issubclass(cls, SocialAbstractRecommender)
    import neurec_amd.model.social_recommender.SBPR as module
    for phrase in ("Deviation, on purpose", "KeyError", "divides by zero", "string form", "WITHOUT the bias"):
        assert phrase in module.__doc__, phrase
    monkeypatch.setattr(AbstractRecommender, "__init__", lambda self, dataset, conf: None)
    path = os.path.join(str(tmp_path), "toy.uu")
    with open(path, "w") as f:
        f.write("a,b\nb,c\nb,c\nz,a\n")
    conf = dict(defaults.MODELS["SBPR"])
    conf.update({"social_file": path, "data.convert.separator": ","})
    conf = {k: v for k, v in conf.items()}
    conf.update(learning_rate=0.001, embedding_size=16, num_epochs=500, reg_mf=0.01, batch_size=512, stddev=0.01,
                verbose=1)
    model = cls(None, _Dataset({"a": 0, "b": 1, "c": 2}), conf)
    assert model.social_matrix.shape == (3, 3) and model.social_matrix.indices.tolist() == [1, 2]
    assert (model.num_epochs, model.batch_size, model.embedding_size, model.reg_mf) == (500, 512, 16, 0.01)
    assert model.learner == "adam" and model.loss_function == "bpr" and model.init_method == "normal"
    assert model.engine is None


def test_defaults_are_written_for_sbpr(tmp_path):
    """defaults.MODELS["SBPR"] holds the values of the reference's conf/SBPR.properties, written as an ini file that
    the Configurator reads back"""
    from neurec_amd import defaults
    path = defaults.write_default_configs(str(tmp_path))
    parser = configparser.ConfigParser()
    parser.optionxform = str
    parser.read(os.path.join(str(tmp_path), "conf", "SBPR.properties"))
    want = {"learning_rate": "0.001", "embedding_size": "16", "learner": "adam", "loss_function": "bpr",
            "num_epochs": "500", "reg_mf": "0.01", "batch_size": "512", "social_file": "dataset/Ciao_u5_s2.uu",
            "init_method": "normal", "stddev": "0.01", "verbose": "1"}
    assert dict(parser["hyperparameters"]) == want
    from neurec_amd.util.configurator import Configurator
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=SBPR"])
    finally:
        os.chdir(cwd)
    assert conf["recommender"] == "SBPR" and conf["num_epochs"] == 500 and conf["batch_size"] == 512
    assert conf["embedding_size"] == 16 and conf["reg_mf"] == 0.01 and conf["social_file"] == "dataset/Ciao_u5_s2.uu"


def test_synthetic_trust_graph_is_seeded():
    from neurec_amd import synth
    has = np.ones(500, bool)
    has[::13] = False
    S = synth.trust_graph(500, seed=5, has_items=has)
    T = synth.trust_graph(500, seed=5, has_items=has)
    assert S.shape == (500, 500) and (S != T).nnz == 0 and (S != synth.trust_graph(500, seed=6, has_items=has)).nnz
    deg = np.diff(S.indptr)
    assert np.all(deg[::11] == 0) and deg.max() > 5 and has[S.indices].all() and S.has_sorted_indices


# ------------------------------------------------------------------ the C entries
def test_the_header_declares_the_entries_and_lib_binds_them():
    from neurec_amd import _lib
    with open(os.path.join(ROOT, "include", "neurec_hip.h")) as f:
        text = f.read()
    for name in ("nrhip_sbpr_expansion_sizes", "nrhip_sbpr_sets_block", "nrhip_sbpr_stream", "nrhip_sbpr_step"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SIGNATURES
    assert re.search(r"#define NRHIP_SBPR_MAX_D 128\b", text) and re.search(r"#define NRHIP_ABI_VERSION 4\b", text)
    for struct, cls, tail in (
            ("nrhip_sbpr_step_args", _lib.SbprStepArgs, ["n_users", "n_items", "d", "batch", "loss_kind", "reg"]),
            ("nrhip_sbpr_sets_args", _lib.SbprSetsArgs, ["n_users", "n_items", "u0", "u1", "n_pairs", "max_seg_len",
                                                        "n_big"]),
            ("nrhip_sbpr_stream_args", _lib.SbprStreamArgs, ["n_slots", "out_begin", "out_count", "seed", "epoch",
                                                             "n_elig", "n_users", "n_items", "shuffle"])):
        block = text[text.index("typedef struct %s" % struct):text.index("} %s;" % struct)]
        pointers = re.findall(r"\*\s*[dh]_(\w+);", block)
        fields = [n for n, _ in cls._fields_]
        assert fields[:len(pointers)] == pointers and fields[len(pointers):] == tail, struct
    from neurec_amd.sbpr import MAX_D, MAX_PAIRS, SEGMENT_PAIRS
    assert MAX_D == 128 and re.search(r"#define NRHIP_SBPR_MAX_PAIRS \(1ll << 30\)", text) and MAX_PAIRS == 1 << 30
    assert re.search(r"#define NRHIP_SBPR_SEGMENT_PAIRS %d\b" % SEGMENT_PAIRS, text)


def test_the_c_entries_refuse_by_name():
    """the bounds of the C entries (host code of the library: no GPU needed, nothing is launched)"""
    from neurec_amd import _lib
    a = _lib.SbprStepArgs()
    a.n_users, a.n_items, a.d, a.batch, a.loss_kind = 5, 6, 129, 0, 0
    with pytest.raises(NotImplementedError, match=r"embedding_size 129 outside 1\.\.128"):
        _lib.call("nrhip_sbpr_step", C.byref(a), None)
    a.d, a.loss_kind = 4, 7
    with pytest.raises(ValueError, match="unknown pairwise loss 7"):
        _lib.call("nrhip_sbpr_step", C.byref(a), None)
    a.loss_kind = 0
    _lib.call("nrhip_sbpr_step", C.byref(a), None)                   # batch == 0: no pointer is needed, no launch
    s = _lib.SbprSetsArgs()
    s.n_users, s.n_items, s.u0, s.u1, s.n_pairs = 5, 6, 3, 2, 0
    with pytest.raises(ValueError, match=r"bad sizes \(users \[3, 2\) of 5"):
        _lib.call("nrhip_sbpr_sets_block", C.byref(s), None)
    s.u0, s.u1, s.n_pairs = 0, 5, (1 << 30) + 1
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.call("nrhip_sbpr_sets_block", C.byref(s), None)
    e = _lib.SbprStreamArgs()
    e.n_items, e.n_slots, e.out_begin, e.out_count = 6, 10, 8, 3
    with pytest.raises(ValueError, match=r"bad range \[8,\+3\) of 10"):
        _lib.call("nrhip_sbpr_stream", C.byref(e), None)
    e.out_count = 0
    _lib.call("nrhip_sbpr_stream", C.byref(e), None)
