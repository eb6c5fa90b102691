"""NPE without a GPU: the float64 restatement the GPU tests lean on (tests/npe_restatement.py) against the reference
class's own f64 trace, the planted zeros and duplicate patterns the golden batches were built to hold, the strict ReLU
gate, the defaults and the dispatch of `recommender=NPE`."""
import configparser
import os

import numpy as np
import pytest

from conftest import load_golden
import npe_restatement as P
from npe_restatement import CASES


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_npe")


def test_the_cases_the_trace_was_recorded_for(golden):
    """both losses x adam at L = 3, square x each row learner at L = 3, one case at L = 2 and one at L = 5; none at
    L = 1 (deviation b); 2 steps each, 3 for the predict case, B <= 64, d = 16"""
    g = golden
    assert sorted(g["cases"].tolist()) == sorted(CASES)
    have = set(CASES.values())
    assert {("cross_entropy", "adam", 3), ("square", "adam", 3)} <= have
    assert {("square", ln, 3) for ln in ("gd", "adagrad", "rmsprop", "momentum")} <= have
    assert {L for _, _, L in have} == {2, 3, 5}
    for case in CASES:
        steps = len(g[case + "_users"])
        assert steps == (3 if case == P.PREDICT_CASE else 2) and g[case + "_users"].shape[1] <= 64
    assert g["P_0"].shape[1] == g["V_0"].shape[1] == g["W_0"].shape[1] == 16 and g["V_0"].shape == g["W_0"].shape


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_the_f64_trace(golden, case):
    """every step of every case: tables and loss within 1e-12 of the reference class's float64 run; predict() after
    the case it was recorded for, full and candidate mode"""
    g = golden
    loss, learner, L = CASES[case]
    st = P.State(g["P_0"], g["V_0"], g["W_0"], learner=learner, lr=float(g["learning_rate"]))
    assert g[case + "_recents"].shape[1:] == (len(g[case + "_users"][0]), L)
    for k in range(len(g[case + "_users"])):
        got = P.step(st, g[case + "_users"][k], g[case + "_recents"][k], g[case + "_items"][k], g[case + "_labels"][k],
                     loss, float(g["reg"]))
        assert abs(got - g[case + "_f64_loss"][k]) <= 1e-12 * max(1.0, abs(got)), (k, got)
        for name, want in zip(P.TABLES, P.golden_tables(g, case, "f64", k)):
            err = np.abs(st.var[name] - want).max()
            assert err <= 1e-12, (case, k, name, err)
    if case == P.PREDICT_CASE:
        seqs = P.sequences(g)
        last = P.last_items_table(seqs, int(g["shape"][0]), L)
        users = g["predict_users"]
        got = P.predict(st.var["P"], st.var["V"], st.var["W"], users, last)
        assert np.abs(got - g["predict_f64"]).max() <= 1e-12
        cand = np.stack([got[k][c] for k, c in enumerate(g["predict_cand"])])
        assert np.abs(cand - g["predict_cand_f64"]).max() <= 1e-12
        # the users the rows were recorded for: |R_u| >= L, |R_u| = 2 (sliced to its last 1) and |R_u| = 1
        lens = [len(seqs[int(u)]) for u in users]
        assert max(lens) >= L and 2 in lens and 1 in lens
        assert [(last[int(u)] >= 0).sum() for u in users if len(seqs[int(u)]) == 2] == [1]


def test_batches_hold_the_planted_zeros_and_the_edges(golden):
    """what the golden batches were built for: in every step of every case, on the tables that step looks up and in
    both widths, a column where P[u] is exactly 0, one where V[i] is exactly 0 and one where the context sum is exactly
    0 by cancellation while its members are not; in every batch a user twice, an item that is a target here and a
    recent there and a window with the same item twice among its recents; every other instance is a window of the
    stored sequences, label-0 items outside the user's sequence"""
    g = golden
    seqs = P.sequences(g)
    for case, (_, _, L) in CASES.items():
        for k in range(len(g[case + "_users"])):
            users, recents, items, labels = (g["%s_%s" % (case, f)][k] for f in ("users", "recents", "items", "labels"))
            assert len(users) <= 64 and recents.shape == (len(users), L)
            assert all(P.edge_patterns(users, recents, items).values()), (case, k)
            for tag in ("f32", "f64"):
                zeros = P.zero_counts(*P.golden_tables(g, case, tag, k - 1), users, recents, items)
                assert min(zeros) >= 1, (case, k, tag, zeros)
            # the reserved window of this step, its last L recents
            b = [j for j in range(len(users)) if users[j] == g["zero_users"][k] and items[j] == g["zero_items"][k]]
            assert b and all(recents[j].tolist() == g["zero_recents"][k][5 - L:].tolist() for j in b)
            for b, (u, r, i) in enumerate(zip(users.tolist(), recents.tolist(), items.tolist())):
                s = seqs[u]
                if len(set(r)) < L:                                   # the window with an item twice
                    r = None
                if labels[b] > 0.5:
                    j = s.index(i)
                    assert j >= L and (r is None or s[j - L:j] == r), (case, k, b)
                else:
                    assert i not in s and (r is None or any(s[j - L:j] == r for j in range(L, len(s)))), (case, k, b)


def test_the_gate_is_strict():
    """TF's ReluGrad (features > 0) on hand-made rows: an input that is exactly 0, or -0, passes nothing — neither its
    value nor a derivative — for each of the three gated inputs; a negative context with positive members is shut;
    the regulariser reaches a W row once per occurrence"""
    assert P.relu(np.array([0.0, -0.0, 0.5, -0.5])).tolist() == [0.0, 0.0, 0.5, 0.0]
    assert P.gate(np.array([0.0, -0.0, 0.5, -0.5])).tolist() == [0.0, 0.0, 1.0, 0.0]
    #                 p = 0   v = 0   s = 0   p = -0  s < 0   open
    Pt = np.array([[0.0, 1.0, 1.0, -0.0, 1.0, 1.0]])
    Vt = np.array([[2.0, 0.0, 2.0, 2.0, 2.0, 2.0], [9.0] * 6])
    Wt = np.array([[1.0, 1.0, 0.25, 1.0, 0.5, 0.5], [1.0, 1.0, -0.25, 1.0, -1.0, 0.25]])
    total, GP, GV, GW = P.gradients(Pt, Vt, Wt, [0], [[0, 1]], [0], [0.0], "square", 0.0)
    x = 2.0 * 2.0 + 0.0 + 2.0 * 1.0 + 2.0 * 2.0 + 2.0 * 1.0 + 2.0 * 1.75
    g = 2.0 * x
    assert total == x * x
    assert GP[0].tolist() == [0.0, 0.0, 2 * g, 0.0, 2 * g, 2 * g]
    assert GV[0].tolist() == [2 * g, 0.0, g, 2 * g, g, 1.75 * g] and not GV[1].any()
    assert GW[0].tolist() == GW[1].tolist() == [2 * g, 0.0, 0.0, 2 * g, 0.0, 2 * g]
    # an item twice among the recents takes its derivative and its regulariser twice
    _, _, _, GW2 = P.gradients(Pt, Vt, Wt, [0], [[0, 0]], [0], [0.0], "square", 0.5)
    _, _, _, GW1 = P.gradients(Pt, Vt, 2 * Wt, [0], [[0]], [0], [0.0], "square", 0.0)
    assert np.array_equal(GW2[0], 2 * GW1[0] + 2 * 0.5 * Wt[0]) and not GW2[1].any()


def test_the_library_names_its_limits():
    """the entry points' own checks (NR_REQUIRE): d 1..128, L 1..16, and the shared key space of U + 2 I rows"""
    import ctypes as C
    from neurec_amd import _lib
    a = _lib.NpeStepArgs()
    for f, _ in a._fields_[:18]:
        setattr(a, f, 1 << 20)                                        # addresses: nothing is read before the refusal
    a.n_users, a.n_items, a.d, a.L, a.batch, a.loss_kind = 5, 6, 129, 2, 0, 1
    with pytest.raises(NotImplementedError, match=r"embedding_size 129 outside 1\.\.128"):
        _lib.call("nrhip_npe_step", C.byref(a), None)
    a.d, a.L = 4, 17
    with pytest.raises(NotImplementedError, match=r"high_order 17 outside 1\.\.16"):
        _lib.call("nrhip_npe_step", C.byref(a), None)
    a.L, a.n_users, a.n_items = 2, 3, (1 << 30) - 2                   # 3 + 2 (2^30 - 2) = 2^31 - 1
    with pytest.raises(ValueError, match="2 n_items < 2\\^31 - 1"):
        _lib.call("nrhip_npe_step", C.byref(a), None)
    with pytest.raises(NotImplementedError, match=r"high_order 0 outside 1\.\.16"):
        _lib.call("nrhip_npe_user_factors", 1 << 20, 1 << 20, 5, 6, 4, 0, 1 << 20, None, 0, 1 << 20, 4, None)
    with pytest.raises(NotImplementedError, match=r"embedding_size 0 outside 1\.\.128"):
        _lib.call("nrhip_npe_item_factors", 1 << 20, 6, 0, 1 << 20, None)


def test_find_recommender_resolves_npe():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import SeqAbstractRecommender
    cls = find_recommender("NPE")
    assert cls.__name__ == "NPE" and cls.__module__ == "neurec_amd.model.sequential_recommender.NPE"
    assert issubclass(cls, SeqAbstractRecommender)


def test_defaults_are_written_for_npe(tmp_path):
    """defaults.MODELS["NPE"] holds the values of the reference's conf/NPE.properties and is written as an ini file"""
    from neurec_amd import defaults
    defaults.write_default_configs(str(tmp_path))
    parser = configparser.ConfigParser()
    parser.optionxform = str
    parser.read(os.path.join(str(tmp_path), "conf", "NPE.properties"))
    got = dict(parser["hyperparameters"])
    assert got == {"epochs": "100", "batch_size": "256", "embedding_size": "64", "reg": "0.1",
                   "learning_rate": "0.001", "learner": "adam", "high_order": "3", "num_neg": "4",
                   "loss_function": "cross_entropy", "init_method": "tnormal", "stddev": "0.01", "verbose": "1"}
