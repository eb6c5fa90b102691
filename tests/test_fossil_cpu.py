"""Fossil without a GPU: the float64 restatement the GPU tests lean on (tests/fossil_restatement.py) against the
reference class's own f64 trace, what the golden pattern and batches hold, the order of the recents the plugin hands
the engine, the per-user table of last items, and the dispatch of `recommender=Fossil`."""
import numpy as np
import pytest

from conftest import load_golden
import fossil_restatement as P
from fossil_restatement import CASES


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_fossil")


def _batch(g, case, k):
    return tuple(g["%s_%s" % (case, f)][k] for f in ("users", "recents", "items", "third"))


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_the_f64_trace(golden, case):
    """every step of every case: the five tables and the loss within 1e-12 of the reference class's float64 run"""
    g = golden
    loss, learner, pairwise, L, regs, alpha = CASES[case]
    R = P.golden_matrix(g)
    st = P.State(*P.initial_tables(g, case), learner=learner, lr=float(g["learning_rate"]))
    for k in range(len(g[case + "_users"])):
        got = P.step(st, R, *_batch(g, case, k), pairwise, loss, alpha, regs)
        assert abs(got - g[case + "_f64_loss"][k]) <= 1e-12 * max(1.0, abs(got)), (k, got)
        for name, want in zip(P.TABLES, P.golden_tables(g, case, "f64", k)):
            err = np.abs(st.var[name] - want).max()
            assert err <= 1e-12, (case, k, name, err)
    if case == "bpr_adagrad":
        seqs = P.sequences(g)
        last = P.last_items(seqs, int(g["shape"][0]), L)
        users = g["predict_users"]
        got = P.predict(R, *[st.var[n] for n in P.TABLES], users, alpha, last)
        assert np.abs(got - g["predict_f64"]).max() <= 1e-12
        cand = np.stack([got[k][c] for k, c in enumerate(g["predict_cand"])])
        assert np.abs(cand - g["predict_cand_f64"]).max() <= 1e-12
        # deviation 2 shows in the rows: a user whose last L items are not a palindrome scores differently with eta
        # column 0 at the most recent item
        flipped = last.copy()
        flipped[users] = flipped[users][:, ::-1]
        other = P.predict(R, *[st.var[n] for n in P.TABLES], users, alpha, flipped)
        assert np.abs(other - g["predict_f64"]).max() > 1e-6
        lens = sorted(len(seqs[int(u)]) for u in users)
        assert lens[0] == L and lens[1] == L + 1 and lens[2] > L + 1


def test_pattern_and_batches_hold_the_edges(golden):
    """the train pattern holds users with |R_u| = 0, < L, = L and = L + 1 (L = 3); every batch of every case holds a
    user twice, a target twice, an item that is a recent here and a target there, and one item at two eta columns of
    two instances of one user; the instances are windows of the stored sequences, recents most recent first"""
    g = golden
    seqs = P.sequences(g)
    deg = np.diff(g["indptr"])
    assert all((deg == n).any() for n in (0, 2, 3, 4))
    for u, s in seqs.items():
        assert sorted(s) == g["indices"][g["indptr"][u]:g["indptr"][u + 1]].tolist()
    for case, (_, _, pairwise, L, _, _) in CASES.items():
        for k in range(len(g[case + "_users"])):
            users, recents, items, third = _batch(g, case, k)
            assert len(users) <= 64 and recents.shape == (len(users), L)
            pat = P.edge_patterns(users, recents, items, third, pairwise)
            assert all(pat.values()), (case, k, pat)
            for b, (u, i) in enumerate(zip(users.tolist(), items.tolist())):
                s = seqs[u]
                assert len(s) > L
                if pairwise or third[b] > 0.5:
                    idx = s.index(i)
                    assert idx >= L and recents[b].tolist() == [s[idx - 1 - l] for l in range(L)], (case, k, b)
                else:
                    assert i not in s and set(recents[b].tolist()) <= set(s), (case, k, b)
                if pairwise:
                    assert int(third[b]) not in s


SEQS = {0: [3, 1, 4, 11, 5, 9], 1: [9, 2], 2: [6], 3: [5, 3, 8, 0, 7, 10, 2], 5: [2, 11, 1, 4]}


@pytest.mark.parametrize("L", [1, 2, 3])
def test_recents_reach_the_engine_most_recent_first(L):
    """the window table behind the time-order samplers (data/streams.py: InstanceRows at high_order = L) delivers
    seq[idx-L..idx-1] ascending; `recents_for_engine` hands the engine [B, L] with column l = seq[idx-1-l] — numpy
    arrays and torch tensors alike"""
    import torch
    from neurec_amd.data.streams import InstanceRows
    from neurec_amd.model.sequential_recommender.Fossil import recents_for_engine
    rows = InstanceRows(SEQS, L, 12)
    users, pos, rec = rows.users(), rows.positives(), rows.recents()
    assert len(users) == sum(max(len(s) - L, 0) for s in SEQS.values()) > 0
    got = recents_for_engine(np.asarray(rec), L)
    got_t = recents_for_engine(torch.from_numpy(np.ascontiguousarray(rec)), L)
    assert got.shape == (len(users), L) and got.flags["C_CONTIGUOUS"] and got_t.is_contiguous()
    assert np.array_equal(got_t.numpy(), got)
    for b in range(len(users)):
        s = SEQS[int(users[b])]
        idx = s.index(int(pos[b]))
        assert idx >= L and got[b].tolist() == [s[idx - 1 - l] for l in range(L)], (b, got[b], s)
        assert np.asarray(rec).reshape(len(users), L)[b].tolist() == s[idx - L:idx]


def test_last_items_table_follows_the_predict_deviations():
    """deviation 2: eta column 0 meets the OLDEST of the last L items; deviation 3: a user with fewer than L items has
    them ascending from column 0 and -1 behind, a user without train items -1 everywhere"""
    from neurec_amd.model.sequential_recommender.Fossil import last_items_table
    last = last_items_table(SEQS, 6, 3)
    assert last.dtype == np.int32 and last.shape == (6, 3)
    assert last.tolist() == [[11, 5, 9], [9, 2, -1], [6, -1, -1], [7, 10, 2], [-1, -1, -1], [11, 1, 4]]
    assert np.array_equal(last, P.last_items(SEQS, 6, 3))
    assert last_items_table(SEQS, 6, 1).reshape(-1).tolist() == [9, 2, 6, 2, -1, 4]


def test_find_recommender_resolves_fossil():
    from neurec_amd import defaults
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import SeqAbstractRecommender
    cls = find_recommender("Fossil")
    assert cls.__name__ == "Fossil" and cls.__module__ == "neurec_amd.model.sequential_recommender.Fossil"
    assert issubclass(cls, SeqAbstractRecommender)
    keys = dict(defaults.MODELS["Fossil"])
    assert keys["high_order"] == "3" and keys["regs"].count(",") == 2 and keys["learner"] == "adagrad"
