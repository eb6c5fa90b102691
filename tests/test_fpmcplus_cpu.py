"""FPMCplus without a GPU: the float64 restatement the GPU tests lean on (tests/fpmcplus_restatement.py) against the
reference class's own f64 trace and against torch.autograd, the duplicate patterns the golden batches were built to
hold, the C entries' refusals, the defaults and the dispatch of `recommender=FPMCplus`."""
import configparser
import os

import numpy as np
import pytest

from conftest import load_golden
import fpmcplus_restatement as P
from fpmcplus_restatement import CASES


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_fpmcplus")


def _batch(g, case, k):
    return tuple(g["%s_%s" % (case, f)][k] for f in ("users", "recents", "items", "third"))


def test_the_cases_the_trace_was_recorded_for(golden):
    """pairwise bpr / adam at L = 3 (the shipped configuration, the predict case), hinge / gd at L = 2, square / rmsprop
    at L = 5; pointwise cross_entropy / adagrad at L = 3 and square / momentum at L = 2; 2 steps each, 3 for the predict
    case, B = 60, d = w = 16; h starts as ones in the shipped case and near 1 elsewhere"""
    g = golden
    assert sorted(g["cases"].tolist()) == sorted(CASES)
    assert set(CASES.values()) == {("bpr", "adam", True, 3), ("hinge", "gd", True, 2), ("square", "rmsprop", True, 5),
                                   ("cross_entropy", "adagrad", False, 3), ("square", "momentum", False, 2)}
    for case, (_, _, pairwise, L) in CASES.items():
        steps = len(g[case + "_users"])
        assert steps == (3 if case == P.PREDICT_CASE else 2)
        assert g[case + "_users"].shape == (steps, 60) and g[case + "_recents"].shape == (steps, 60, L)
        assert g[case + "_third"].dtype == (np.int32 if pairwise else np.float32)
    assert tuple(int(x) for x in g["shape"]) == (157, 131)
    assert g["UI_0"].shape == (157, 16) and g["W_0"].shape == (48, 16) and g["b_0"].shape == (1, 16)
    assert np.all(g[P.PREDICT_CASE + "_h_0"] == 1)
    others = [c for c in CASES if c != P.PREDICT_CASE]
    assert all(np.all(g[c + "_h_0"] != 1) and np.abs(g[c + "_h_0"] - 1).max() < 0.5 for c in others)


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_the_f64_trace(golden, case):
    """every step of every case: the seven tables and the loss within 1e-12 (relative to max(1, |want|)) of the
    reference class's float64 run; predict() after the case it was recorded for, full and candidate mode"""
    g = golden
    loss, learner, pairwise, L = CASES[case]
    st = P.State(*P.golden_tables(g, case, "f64", -1), learner=learner, lr=float(g["learning_rate"]))
    for k in range(len(g[case + "_users"])):
        got = P.step(st, *_batch(g, case, k), pairwise, loss, float(g["reg_mf"]), float(g["reg_w"]))
        want = g[case + "_f64_loss"][k]
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (k, got, want)
        for name, want in zip(P.TABLES, P.golden_tables(g, case, "f64", k)):
            err = np.abs(st.var[name] - want).max()
            assert err <= 1e-12 * max(1.0, np.abs(want).max()), (case, k, name, err)
    if case == P.PREDICT_CASE:
        seqs = P.sequences(g)
        last = P.last_items_table(seqs, int(g["shape"][0]), L)
        users = g["predict_users"]
        assert all(len(seqs[int(u)]) >= L for u in users)
        got = P.predict(*st.tables(), users, last)
        assert np.abs(got - g["predict_f64"]).max() <= 1e-12
        cand = np.stack([got[k][c] for k, c in enumerate(g["predict_cand"])])
        assert np.abs(cand - g["predict_cand_f64"]).max() <= 1e-12


def _autograd(tabs, users, recents, items, third, pairwise, loss, reg_mf, reg_w):
    """the loss of FPMCplus.py:73-119 written with torch ops in float64, present slots only, and its gradients"""
    import torch
    UI, IU, IL, LI, W, b, h = (torch.tensor(np.asarray(t, np.float64), requires_grad=True) for t in tabs)
    d = UI.shape[1]
    u, i = torch.as_tensor(users, dtype=torch.long), torch.as_tensor(items, dtype=torch.long)
    rec = torch.as_tensor(np.asarray(recents), dtype=torch.long)
    present = (rec >= 0).double()
    rows = LI[rec.clamp(min=0)] * present[:, :, None]

    def x_of(it):
        z = torch.cat([UI[u][:, None, :].expand(-1, rec.shape[1], -1), IL[it][:, None, :].expand(-1, rec.shape[1], -1),
                       rows], dim=2)
        a = torch.tanh(z.reshape(-1, 3 * d) @ W + b[None, :])
        ex = torch.exp((a @ h).reshape(rec.shape)) * present
        tot = ex.sum(dim=1, keepdim=True)
        alpha = torch.where(tot > 0, ex / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.zeros_like(ex))
        s = (alpha[:, :, None] * rows).sum(dim=1)
        return (UI[u] * IU[it]).sum(dim=1) + (IL[it] * s).sum(dim=1)
    l2 = lambda *ts: sum((t ** 2).sum() for t in ts) / 2
    x = x_of(i)
    if pairwise:
        j = torch.as_tensor(np.asarray(third), dtype=torch.long)
        y = x - x_of(j)
        main = {"bpr": lambda: -torch.nn.functional.logsigmoid(y).sum(),
                "hinge": lambda: torch.clamp(y + 1, min=0).sum(), "square": lambda: ((1 - y) ** 2).sum()}[loss]()
        total = main + reg_mf * l2(UI[u], IU[i], IL[i], rows, IU[j], IL[j]) + reg_w * l2(W, h)
    else:
        z = torch.as_tensor(np.asarray(third, np.float64))
        main = ((z - x) ** 2).sum() if loss == "square" else \
            torch.nn.functional.binary_cross_entropy_with_logits(x, z, reduction="mean")
        total = main + reg_mf * l2(UI[u], IU[i], IL[i], rows)
    total.backward()
    return float(total.detach()), [t.grad.numpy() for t in (UI, IU, IL, LI, W, b, h)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_hand_gradients_match_autograd(golden, case):
    """torch.autograd in float64 against the restatement's hand gradients, all seven tables, on the first batch of
    every case and on the same batch with absent slots (-1) mixed in and one instance with none present: 1e-13
    (relative to max(1, |want|)), the bound of test_dense_cpu.py"""
    g = golden
    loss, _, pairwise, L = CASES[case]
    tabs = P.golden_tables(g, case, "f64", -1)
    users, recents, items, third = _batch(g, case, 0)
    holes = recents.copy()
    holes[3, 0] = holes[5, L - 1] = -1
    holes[7, :] = -1
    for rec in (recents, holes):
        want_loss, want = _autograd(tabs, users, rec, items, third, pairwise, loss, 0.01, 0.02)
        got_loss, G = P.gradients(*tabs, users, rec, items, third, pairwise, loss, 0.01, 0.02)
        assert abs(got_loss - want_loss) <= 1e-13 * max(1.0, abs(want_loss))
        for name, w in zip(P.TABLES, want):
            err = np.abs(G[name] - w.reshape(G[name].shape)).max()
            assert err <= 1e-13 * max(1.0, np.abs(w).max()), (case, name, err)
            assert np.abs(w).max() > 0, name


def test_batches_hold_the_edges(golden):
    """in every batch a user twice, an item that is a target here and a recent there, an instance with the same item
    twice among its recents and, pairwise, a negative that is another instance's positive"""
    g = golden
    for case, (_, _, pairwise, L) in CASES.items():
        for k in range(len(g[case + "_users"])):
            pat = P.edge_patterns(*_batch(g, case, k), pairwise)
            assert len(pat) == (4 if pairwise else 3) and all(pat.values()), (case, k, pat)


def test_the_score_does_not_depend_on_the_order_of_the_recents(golden):
    g = golden
    case = "square_rmsprop"
    tabs = P.golden_tables(g, case, "f64", -1)
    users, recents, items, _ = _batch(g, case, 0)
    x = P.scores(*tabs, users.astype(np.int64), items.astype(np.int64), recents.astype(np.int64))
    xr = P.scores(*tabs, users.astype(np.int64), items.astype(np.int64), recents[:, ::-1].astype(np.int64))
    assert np.abs(x - xr).max() <= 1e-15


def test_the_c_entries_refuse_by_name():
    """the bounds of the C entries (host code of the library: no GPU needed, nothing is launched)"""
    import ctypes as C
    from neurec_amd import _lib
    a = _lib.FpmcplusStepArgs()
    a.n_users, a.n_items, a.d, a.w, a.L, a.batch, a.pairwise, a.loss_kind = 5, 6, 129, 4, 2, 0, 1, 0
    with pytest.raises(NotImplementedError, match=r"embedding_size 129 outside 1\.\.128"):
        _lib.call("nrhip_fpmcplus_step", C.byref(a), None)
    a.d, a.w = 4, 65
    with pytest.raises(NotImplementedError, match=r"weight_size 65 outside 1\.\.64"):
        _lib.call("nrhip_fpmcplus_step", C.byref(a), None)
    a.w, a.L = 4, 17
    with pytest.raises(NotImplementedError, match=r"high_order 17 outside 1\.\.16"):
        _lib.call("nrhip_fpmcplus_step", C.byref(a), None)
    a.L = 0
    with pytest.raises(NotImplementedError, match=r"high_order 0 outside 1\.\.16"):
        _lib.call("nrhip_fpmcplus_step", C.byref(a), None)
    a.L, a.loss_kind = 2, 7
    with pytest.raises(ValueError, match="unknown pairwise loss 7"):
        _lib.call("nrhip_fpmcplus_step", C.byref(a), None)
    a.loss_kind = 0
    _lib.call("nrhip_fpmcplus_step", C.byref(a), None)               # batch == 0: no pointer is needed, no launch
    s = _lib.FpmcplusScoresArgs()
    s.n_users, s.n_items, s.d, s.w, s.L, s.batch, s.ld = 5, 6, 4, 65, 2, 0, 6
    with pytest.raises(NotImplementedError, match=r"weight_size 65 outside 1\.\.64"):
        _lib.call("nrhip_fpmcplus_scores", C.byref(s), None)
    s.w = 4
    _lib.call("nrhip_fpmcplus_scores", C.byref(s), None)


def test_find_recommender_resolves_fpmcplus():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import SeqAbstractRecommender
    cls = find_recommender("FPMCplus")
    assert cls.__name__ == "FPMCplus" and cls.__module__ == "neurec_amd.model.sequential_recommender.FPMCplus"
    assert issubclass(cls, SeqAbstractRecommender)


def test_defaults_are_written_for_fpmcplus(tmp_path):
    """defaults.MODELS["FPMCplus"] holds the values of the reference's conf/FPMCplus.properties, written as an ini file"""
    from neurec_amd import defaults
    defaults.write_default_configs(str(tmp_path))
    parser = configparser.ConfigParser()
    parser.optionxform = str
    parser.read(os.path.join(str(tmp_path), "conf", "FPMCplus.properties"))
    got = dict(parser["hyperparameters"])
    assert got == {"epochs": "500", "batch_size": "128", "embedding_size": "16", "weight_size": "16", "high_order": "3",
                   "reg_mf": "0.00001", "reg_w": "0.001", "learning_rate": "0.001", "learner": "adam",
                   "is_pairwise": "True", "num_neg": "4", "loss_function": "BPR", "embed_init_method": "tnormal",
                   "weight_init_method": "he_normal", "stddev": "0.01", "verbose": "1"}
