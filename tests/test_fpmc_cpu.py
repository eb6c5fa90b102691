"""FPMC without a GPU: the float64 restatement the GPU tests lean on (tests/fpmc_restatement.py) against the reference
class's own f64 trace, the duplicate patterns of the golden batches, the sequential base class and the dispatch of
`recommender=FPMC`."""
import numpy as np
import pytest

from conftest import load_golden
import fpmc_restatement as P
from fpmc_restatement import CASES


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_fpmc")


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_the_f64_trace(golden, case):
    """every step of every case: tables and loss within 1e-12 of the reference class's float64 run"""
    g = golden
    loss, learner, pairwise = CASES[case]
    st = P.State(g["UI_0"], g["IU_0"], g["IL_0"], g["LI_0"], learner=learner, lr=float(g["learning_rate"]))
    for k in range(len(g[case + "_users"])):
        got = P.step(st, g[case + "_users"][k], g[case + "_recent"][k], g[case + "_items"][k], g[case + "_third"][k],
                     pairwise, loss, float(g["reg_mf"]))
        assert abs(got - g[case + "_f64_loss"][k]) <= 1e-12 * max(1.0, abs(got)), (k, got)
        for name, want in zip(P.TABLES, P.golden_tables(g, case, "f64", k)):
            err = np.abs(st.var[name] - want).max()
            assert err <= 1e-12, (case, k, name, err)
    if case == "ce_adam":
        seqs = P.sequences(g)
        last = P.last_items(seqs, int(g["shape"][0]))
        users = g["predict_users"]
        got = P.predict(*[st.var[n] for n in P.TABLES], users, last)
        assert np.abs(got - g["predict_f64"]).max() <= 1e-12
        cand = np.stack([got[k][c] for k, c in enumerate(g["predict_cand"])])
        assert np.abs(cand - g["predict_cand_f64"]).max() <= 1e-12
        # the users the rows were recorded for: one whose most recent item is not its largest item id
        assert any(seqs[int(u)][-1] != max(seqs[int(u)]) for u in users)


def test_batches_hold_the_edges(golden):
    """what the golden batches were chosen for, in every batch of every case: a user twice, an item twice as target,
    an item twice as recent, an item that is recent in one instance and the target of another, and an item that is
    positive here and negative there (pairwise) / label 1 here and label 0 there (pointwise); the instances are
    windows of the stored sequences, negatives and label-0 items outside the user's sequence"""
    g = golden
    seqs = P.sequences(g)
    assert sum(1 for s in seqs.values() if len(s) > 1 and s[-1] != max(s)) > len(seqs) // 2
    for case, (_, _, pairwise) in CASES.items():
        for k in range(len(g[case + "_users"])):
            users, recent, items, third = (g["%s_%s" % (case, f)][k] for f in ("users", "recent", "items", "third"))
            assert len(users) <= 64
            pat = P.edge_patterns(users, recent, items, third, pairwise)
            assert all(pat.values()), (case, k, pat)
            for b, (u, l, i) in enumerate(zip(users.tolist(), recent.tolist(), items.tolist())):
                s = seqs[u]
                if pairwise or third[b] > 0.5:
                    assert s[s.index(i) - 1] == l and s.index(i) > 0, (case, k, b)
                else:
                    assert i not in s and l in s[:-1], (case, k, b)
                if pairwise:
                    assert int(third[b]) not in s


def test_sequential_base_class_needs_timestamps():
    """AbstractRecommender.py:48-52: raised before anything else is built"""
    from neurec_amd.model.AbstractRecommender import AbstractRecommender, SeqAbstractRecommender
    assert issubclass(SeqAbstractRecommender, AbstractRecommender)
    ds = type("DS", (), {"time_matrix": None})()
    with pytest.raises(ValueError, match="Dataset does not contant time infomation!"):
        SeqAbstractRecommender(ds, {})


def test_find_recommender_resolves_fpmc():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import SeqAbstractRecommender
    cls = find_recommender("FPMC")
    assert cls.__name__ == "FPMC" and cls.__module__ == "neurec_amd.model.sequential_recommender.FPMC"
    assert issubclass(cls, SeqAbstractRecommender)
