"""FISM without a GPU: the float64 restatement the GPU tests lean on (tests/fism_restatement.py) against the reference
class's own f64 trace, the reference generator's instance structure, and the (history, count) rule on that structure.
(The triples of PointwiseSampler are checked in test_fism_gpu.py: the sampler forms its epoch on the device.)"""
import numpy as np
import pytest

from conftest import load_golden
import fism_restatement as F

CASES = {"square_adam": ("square", "adam", False), "ce_adam": ("cross_entropy", "adam", False),
         "square_gd": ("square", "gd", False), "square_adagrad": ("square", "adagrad", False),
         "square_rmsprop": ("square", "rmsprop", False), "square_momentum": ("square", "momentum", False),
         "bpr_adam": ("bpr", "adam", True)}


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_fism")


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_the_f64_trace(golden, case):
    """every step of every case: tables and loss within 1e-12 of the reference class's float64 run"""
    g = golden
    loss, learner, pairwise = CASES[case]
    R = F.golden_matrix(g)
    st = F.State(g["c1_0"], g["Q0"], g["bias_0"], learner=learner, lr=float(g["learning_rate"]))
    for k in range(len(g[case + "_users"])):
        got = F.step(st, R, g[case + "_users"][k], g[case + "_items"][k], g[case + "_third"][k], pairwise, loss,
                     float(g["alpha"]), g["regs"])
        assert abs(got - g[case + "_f64_loss"][k]) <= 1e-12 * max(1.0, abs(got)), (k, got)
        for name, want in zip(("c1", "Q", "bias"), F.golden_tables(g, case, "f64", k)):
            err = np.abs(st.var[name] - want).max()
            assert err <= 1e-12, (case, k, name, err)
    if case == "square_adam":
        got = F.predict(R, st.var["c1"], st.var["Q"], st.var["bias"], g["predict_users"], float(g["alpha"]))
        assert np.abs(got - g["predict_f64"]).max() <= 1e-12
        got0 = F.predict(R, g["c1_0"], g["Q0"], g["bias_0"], g["predict_users"], 0.0)
        assert np.abs(got0 - g["predict0_f64"]).max() <= 1e-12


def test_batches_hold_the_edges(golden):
    """what the golden batches were chosen for: a user twice, an item twice, excluded first / last of the row, an empty
    history, histories of 1, 63, 64, 65 and 1,100 items"""
    g = golden
    R = F.golden_matrix(g)
    for case, (_, _, pairwise) in CASES.items():
        lens_all = set()
        for k in range(len(g[case + "_users"])):
            inst = F.instances(R, g[case + "_users"][k], g[case + "_items"][k], g[case + "_third"][k], pairwise)
            assert len(inst) <= 64
            users, items = [x[0] for x in inst], [x[1] for x in inst]
            assert len(set(users)) < len(users) and len(set(items)) < len(items)
            lens = {len(F.history(R, u, e)) for u, _, e, _, _ in inst}
            assert {1, 63, 64, 65} <= lens and (pairwise or 0 in lens)
            first = [1 for u, _, e, _, _ in inst if e >= 0 and R.indices[R.indptr[u]] == e]
            last = [1 for u, _, e, _, _ in inst if e >= 0 and R.indices[R.indptr[u + 1] - 1] == e]
            assert first and last
            lens_all |= lens
        if case in ("square_adam", "bpr_adam"):
            assert max(lens_all) >= 1099


def test_reference_generator_structure(golden):
    """_get_pointwise_all_likefism_data, per instance: a positive (label 1) pools the row without its item and counts
    n = |R_u|; each of its num_neg negatives (label 0, item outside the row) pools the whole row and counts |R_u| + 1;
    one epoch is nnz (1 + num_neg) instances"""
    g = golden
    indptr, indices = g["struct_indptr"], g["struct_indices"]
    deg = np.diff(indptr)
    u, i, y = g["struct_user"], g["struct_item"], g["struct_label"]
    n, hl, ex = g["struct_num_idx"], g["struct_hist_len"], g["struct_excluded"]
    assert len(u) == indptr[-1] * 5
    rows = [set(indices[indptr[k]:indptr[k + 1]].tolist()) for k in range(len(deg))]
    inrow = np.asarray([int(it) in rows[us] for us, it in zip(u, i)])
    assert np.array_equal(inrow, y == 1)
    pos = y == 1
    assert np.array_equal(n[pos], deg[u[pos]]) and np.array_equal(hl[pos], deg[u[pos]] - 1)
    assert np.array_equal(ex[pos], i[pos])
    assert np.array_equal(n[~pos], deg[u[~pos]] + 1) and np.array_equal(hl[~pos], deg[u[~pos]]) and np.all(ex[~pos] == -1)
    assert np.array_equal(n, hl + 1)                        # during training n = |H| + 1
    assert (pos.sum(), (~pos).sum()) == (indptr[-1], 4 * indptr[-1])
    assert hl[pos & (deg[u] == 1)].max(initial=0) == 0 and (pos & (deg[u] == 1)).any()   # empty history: out = bias[i]


def test_restatement_instances_follow_the_reference_rule(golden):
    """the (user, item, label) -> (history, n) rule of the restatement (and of csrc/fism.hip) on the structure fixture"""
    import scipy.sparse as sp
    g = golden
    R = sp.csr_matrix((np.ones(len(g["struct_indices"]), np.float32), g["struct_indices"], g["struct_indptr"]),
                      shape=tuple(int(x) for x in g["struct_shape"]))
    inst = F.instances(R, g["struct_user"], g["struct_item"], g["struct_label"].astype(np.float32), False)
    assert [x[2] for x in inst] == g["struct_excluded"].tolist()
    assert [x[3] for x in inst] == g["struct_num_idx"].tolist()
    assert [len(F.history(R, x[0], x[2])) for x in inst] == g["struct_hist_len"].tolist()
