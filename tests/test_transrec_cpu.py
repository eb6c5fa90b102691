"""TransRec without a GPU: the float64 restatement the GPU tests lean on (tests/transrec_restatement.py) against the
reference class's own f64 trace, the duplicate patterns the golden batches were built to hold, the ops the golden maker
attaches to the shim, the C entries' declarations and refusals, the defaults and the dispatch of
`recommender=TransRec`."""
import configparser
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from conftest import load_golden
import transrec_restatement as P
from transrec_restatement import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_transrec")


def _batch(g, case, k):
    return tuple(g["%s_%s" % (case, f)][k] for f in ("users", "recent", "items", "third"))


def test_the_cases_the_trace_was_recorded_for(golden):
    """FPMC's seven cases, hinge / adam pairwise and one case without a regulariser; b [I] and T [1, d] beside P and Q"""
    g = golden
    assert sorted(g["cases"].tolist()) == sorted(CASES) and len(CASES) == 9
    assert CASES["hinge_adam"] == ("hinge", "adam", True, P.REG) and CASES["bpr_adam_reg0"][3] == 0.0
    for case, (_, _, pairwise, reg) in CASES.items():
        assert float(g[case + "_reg_mf"]) == reg
        assert g[case + "_third"].dtype == (np.int32 if pairwise else np.float32)
        assert g[case + "_f64_T"].shape == (len(g[case + "_users"]), 1, 16)
    assert tuple(int(x) for x in g["shape"]) == (157, 131)
    assert g["P_0"].shape == (157, 16) and g["Q_0"].shape == (131, 16)
    assert g["b_0"].shape == (131,) and g["T_0"].shape == (1, 16)


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_the_f64_trace(golden, case):
    """every step of every case: the four tables and the loss within 1e-12 of the reference class's float64 run;
    predict() after the case it was recorded for, full and candidate mode"""
    g = golden
    loss, learner, pairwise, reg = CASES[case]
    st = P.State(*P.golden_tables(g, case, "f64", -1), learner=learner, lr=float(g["learning_rate"]))
    for k in range(len(g[case + "_users"])):
        got = P.step(st, *_batch(g, case, k), pairwise, loss, reg)
        want = g[case + "_f64_loss"][k]
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (k, got, want)
        for name, want in zip(P.TABLES, P.golden_tables(g, case, "f64", k)):
            err = np.abs(st.var[name] - want).max()
            assert err <= 1e-12, (case, k, name, err)
        assert np.abs(g[case + "_f64_T"][k]).max() > 0          # T moves in every step
    if case == P.PREDICT_CASE:
        seqs = P.sequences(g)
        last = P.last_items(seqs, int(g["shape"][0]))
        users = g["predict_users"]
        got = P.predict(*st.tables(), users, last)
        assert np.abs(got - g["predict_f64"]).max() <= 1e-12
        cand = np.stack([got[k][c] for k, c in enumerate(g["predict_cand"])])
        assert np.abs(cand - g["predict_cand_f64"]).max() <= 1e-12
        # the users the rows were recorded for: one whose most recent item is not its largest item id
        assert any(seqs[int(u)][-1] != max(seqs[int(u)]) for u in users)


def test_only_looked_up_rows_move(golden):
    """P, Q and b get the sparse application: the rows a case's trace holds are rows its batches looked up — Q's in any
    of its three roles, b's as a target or a negative"""
    g = golden
    for case, (_, _, pairwise, _) in CASES.items():
        seen = {k: set() for k in P.ROWS}
        for k in range(len(g[case + "_users"])):
            for name, rows in P.touched(*_batch(g, case, k), pairwise).items():
                seen[name] |= set(rows.tolist())
        for name in P.ROWS:
            assert set(g["%s_rows_%s" % (case, name)].tolist()) <= seen[name], (case, name)
        assert len(g[case + "_rows_b"]) < len(g[case + "_rows_Q"])     # recents alone move no bias


def test_batches_hold_the_edges(golden):
    """in every batch of every case: a user twice, an item that is a recent here and a target there (pairwise: and a
    negative elsewhere), and an instance whose target is its own recent item"""
    g = golden
    for case, (_, _, pairwise, _) in CASES.items():
        for k in range(len(g[case + "_users"])):
            users, recent, items, third = _batch(g, case, k)
            assert len(users) <= 64
            pat = P.edge_patterns(users, recent, items, third, pairwise)
            assert len(pat) == (4 if pairwise else 3) and all(pat.values()), (case, k, pat)


def _autograd(tabs, users, recent, items, third, pairwise, loss, reg):
    """the loss of TransRec.py:66-91 written with torch ops in float64, and its gradients"""
    import torch
    Pm, Q, b, T = (torch.tensor(np.asarray(t, np.float64), requires_grad=True) for t in tabs)
    u, l, i = (torch.as_tensor(np.asarray(x), dtype=torch.long) for x in (users, recent, items))
    l2 = lambda *ts: sum((t ** 2).sum() for t in ts) / 2

    def x_of(it):
        v = Pm[u] + T[None, :].repeat(len(u), 1) + Q[l] - Q[it]
        return b[it] - (v ** 2).sum(dim=1)
    x = x_of(i)
    if pairwise:
        j = torch.as_tensor(np.asarray(third), dtype=torch.long)
        y = x - x_of(j)
        main = {"bpr": lambda: -torch.nn.functional.logsigmoid(y).sum(),
                "hinge": lambda: torch.clamp(y + 1, min=0).sum(), "square": lambda: ((1 - y) ** 2).sum()}[loss]()
        total = main + reg * l2(Pm[u], Q[l], Q[j], Q[i], b[i], b[j], T)
    else:
        z = torch.as_tensor(np.asarray(third, np.float64))
        main = ((z - x) ** 2).sum() if loss == "square" else \
            torch.nn.functional.binary_cross_entropy_with_logits(x, z, reduction="mean")
        total = main + reg * l2(Pm[u], Q[l], Q[i], b[i], T)
    total.backward()
    return float(total.detach()), [t.grad.numpy() for t in (Pm, Q, b, T)]


@pytest.mark.parametrize("case", ["ce_adam", "square_gd", "bpr_adam", "hinge_adam"])
def test_hand_gradients_match_autograd(golden, case):
    """torch.autograd in float64 against the restatement's hand gradients on the first batch of a case, with an
    instance whose negative is its own target added in the pairwise cases: 1e-13 relative to max(1, |want|)"""
    g = golden
    loss, _, pairwise, _ = CASES[case]
    tabs = P.golden_tables(g, case, "f64", -1)
    users, recent, items, third = (x.copy() for x in _batch(g, case, 0))
    if pairwise:
        third[4] = items[4]
    want_loss, want = _autograd(tabs, users, recent, items, third, pairwise, loss, 0.5)
    got_loss, G = P.gradients(*tabs, users, recent, items, third, pairwise, loss, 0.5)
    assert abs(got_loss - want_loss) <= 1e-13 * max(1.0, abs(want_loss))
    for name, w in zip(P.TABLES, want):
        err = np.abs(G[name] - w).max()
        assert err <= 1e-13 * max(1.0, np.abs(w).max()), (case, name, err)
        assert np.abs(w).max() > 0, name


def test_the_makers_shim_ops():
    """tests/golden/make_golden_transrec.py attaches tile, norm and a stack that takes Python ints to the shim, and
    checks each on a small value; the shim is put back as it was"""
    from oracle import tf_shim
    spec = importlib.util.spec_from_file_location(
        "make_golden_transrec", os.path.join(ROOT, "tests", "golden", "make_golden_transrec.py"))
    path = list(sys.path)
    before = {k: getattr(tf_shim, k, None) for k in ("tile", "norm", "stack")}
    try:
        maker = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(maker)
        assert maker.attach_ops() is True
        assert all(hasattr(tf_shim, k) for k in before)
        assert sorted(maker.P.CASES) == sorted(CASES)
    finally:
        for k, v in before.items():
            if v is None:
                if hasattr(tf_shim, k):
                    delattr(tf_shim, k)
            else:
                setattr(tf_shim, k, v)
        sys.path[:] = path


def test_the_header_declares_the_entries_and_lib_binds_them():
    from neurec_amd import _lib
    with open(os.path.join(ROOT, "include", "neurec_hip.h")) as f:
        text = f.read()
    for name in ("nrhip_transrec_step", "nrhip_transrec_queries", "nrhip_transrec_scores"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SIGNATURES
        above = re.findall(r"^/\*.*?\*/", text[:text.index("int %s(" % name)], re.S | re.M)[-1]
        assert re.search(r"[Rr]eplaces", above) and "TransRec.py:" in above, name         # cites what it replaces
    assert re.search(r"#define NRHIP_TRANSREC_MAX_D 128\b", text)
    assert re.search(r"#define NRHIP_ABI_VERSION 4\b", text)
    block = text[text.index("typedef struct nrhip_transrec_step_args"):text.index("} nrhip_transrec_step_args;")]
    pointers = re.findall(r"\*\s*d_(\w+);", block)
    fields = [n for n, _ in _lib.TransrecStepArgs._fields_]
    assert fields[:len(pointers)] == pointers
    assert fields[len(pointers):] == ["n_users", "n_items", "d", "batch", "pairwise", "loss_kind", "reg"]
    from neurec_amd.transrec import GT_CHUNK, GT_MAX_CHUNKS, MAX_D
    assert re.search(r"#define NRHIP_TRANSREC_CHUNK %d\b" % GT_CHUNK, text)
    assert re.search(r"#define NRHIP_TRANSREC_MAX_CHUNKS %d\b" % GT_MAX_CHUNKS, text) and MAX_D == 128


def test_the_c_entries_refuse_by_name():
    """the bounds of the C entries (host code of the library: no GPU needed, nothing is launched)"""
    from neurec_amd import _lib
    a = _lib.TransrecStepArgs()
    a.n_users, a.n_items, a.d, a.batch, a.pairwise, a.loss_kind = 5, 6, 129, 0, 1, 0
    with pytest.raises(NotImplementedError, match=r"embedding_size 129 outside 1\.\.128"):
        _lib.call("nrhip_transrec_step", C.byref(a), None)
    a.d = 0
    with pytest.raises(NotImplementedError, match=r"embedding_size 0 outside 1\.\.128"):
        _lib.call("nrhip_transrec_step", C.byref(a), None)
    a.d, a.loss_kind = 4, 7
    with pytest.raises(ValueError, match="unknown pairwise loss 7"):
        _lib.call("nrhip_transrec_step", C.byref(a), None)
    a.loss_kind = 0
    _lib.call("nrhip_transrec_step", C.byref(a), None)               # batch == 0: no pointer is needed, no launch
    with pytest.raises(NotImplementedError, match=r"embedding_size 129 outside 1\.\.128"):
        _lib.call("nrhip_transrec_queries", None, None, None, 5, 6, 129, None, None, 0, None, 129, None)
    _lib.call("nrhip_transrec_queries", None, None, None, 5, 6, 4, None, None, 0, None, 4, None)
    with pytest.raises(NotImplementedError, match=r"embedding_size 129 outside 1\.\.128"):
        _lib.call("nrhip_transrec_scores", None, 129, None, None, 0, 6, 129, None, 6, None)
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.call("nrhip_transrec_scores", None, 4, None, None, 3, 6, 4, None, 5, None)       # ld < n_items
    _lib.call("nrhip_transrec_scores", None, 4, None, None, 0, 6, 4, None, 6, None)


def test_find_recommender_resolves_transrec():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import SeqAbstractRecommender
    cls = find_recommender("TransRec")
    assert cls.__name__ == "TransRec" and cls.__module__ == "neurec_amd.model.sequential_recommender.TransRec"
    assert issubclass(cls, SeqAbstractRecommender)


def test_defaults_are_written_for_transrec(tmp_path):
    """defaults.MODELS["TransRec"] holds the values of the reference's conf/TransRec.properties, written as an ini file
    that the Configurator reads back"""
    from neurec_amd import defaults
    path = defaults.write_default_configs(str(tmp_path))
    parser = configparser.ConfigParser()
    parser.optionxform = str
    parser.read(os.path.join(str(tmp_path), "conf", "TransRec.properties"))
    want = {"epochs": "500", "batch_size": "1024", "embedding_size": "50", "reg_mf": "0.0", "learning_rate": "0.001",
            "learner": "adam", "is_pairwise": "True", "num_neg": "4", "loss_function": "bpr", "init_method": "tnormal",
            "stddev": "0.01", "verbose": "1"}
    assert dict(parser["hyperparameters"]) == want
    from neurec_amd.util.configurator import Configurator
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=TransRec"])
    finally:
        os.chdir(cwd)
    assert conf["recommender"] == "TransRec"
    assert conf["batch_size"] == 1024 and conf["embedding_size"] == 50 and conf["reg_mf"] == 0.0
    assert conf["is_pairwise"] is True and conf["loss_function"] == "bpr" and conf["init_method"] == "tnormal"
