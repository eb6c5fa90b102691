"""ItemKNN on the GPU (csrc/itemknn.hip through neurec_amd/itemknn.py): the similarity build against the reference's
recorded columns and against a float64 restatement, tie-aware in every column; the engine's own tie rule; the scoring;
both accumulator forms (LDS, global slab); determinism; the drop-in run through neurec_amd.main; the refusals."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_golden
from neurec_amd import defaults
from test_itemknn_cpu import DATA, SIMILARITIES, dense_f64, golden_matrix, golden_params

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
REL_EXACT = 8 * EPS        # integer co-occurrences are exact in fp32; then sqrt, multiply, two adds, divide and the
#                            reference's final float32 cast, each correctly rounded: a handful of 2^-24 steps


def _engine(R, neighbor, shrink=0, similarity="cosine", **kw):
    from neurec_amd.itemknn import ItemKNNEngine
    return ItemKNNEngine(R, neighbor, shrink, similarity, **kw)


def check_columns(W, dense, cols, K, rel=0.0, atol=0.0, tag=""):
    """Tie-aware comparison of the engine's columns `cols` of W (scipy, W[j, i]) with the float64 columns
    dense[:, k] (column cols[k] before the cut); tolerance rel * |value| + atol.  Returns the largest value error."""
    Wc = sp.csc_matrix(W)
    I = Wc.shape[0]
    K = min(K, I)
    worst = 0.0
    for k, i in enumerate(cols):
        ref = np.nan_to_num(dense[:, k], nan=0.0)
        idx = Wc.indices[Wc.indptr[i]:Wc.indptr[i + 1]]
        val = Wc.data[Wc.indptr[i]:Wc.indptr[i + 1]].astype(np.float64)
        assert np.all(val != 0) and np.all(np.isfinite(val)), (tag, i)          # no stored zeros, NaN or inf
        top = -np.sort(-ref)[:K]
        kth = top[-1]
        tol_k = rel * abs(kth) + atol
        want = top[top != 0]
        sure = int(np.sum(np.abs(top) > rel * np.abs(top) + atol))
        assert sure <= len(val) <= len(want) or len(val) == len(want), (tag, i, len(val), len(want))
        n = min(len(val), len(want))
        got_sorted = -np.sort(-val)
        err = np.abs(got_sorted[:n] - want[:n])
        assert np.all(err <= rel * np.abs(want[:n]) + atol), (tag, i, err.max())
        worst = max(worst, float(err.max()) if n else 0.0)
        assert np.all(ref[idx] >= kth - tol_k), (tag, i)                        # nothing below the K-th value
        must = np.flatnonzero((ref > kth + tol_k) & (np.abs(ref) > atol))
        assert np.isin(must, idx).all(), (tag, i)                               # everything above it
    return worst


def check_scores(eng, R, users, W=None):
    """score(users) against float64 R[users] @ W_engine: |err| <= (n_terms + 1) 2^-24 sum |terms| per element"""
    W = eng.similarity() if W is None else W
    R = sp.csr_matrix(R, dtype=np.float64)
    S = eng.score(np.asarray(users, np.int32)).cpu().numpy()
    assert S.shape == (len(users), R.shape[1]) and S.dtype == np.float32 and np.all(np.isfinite(S))
    W64 = sp.csr_matrix(W, dtype=np.float64)
    Ru = R[users]
    want = np.asarray((Ru @ W64).todense())
    mag = np.asarray((abs(Ru) @ abs(W64)).todense())
    nterm = np.asarray(((Ru != 0).astype(np.float64) @ (W64 != 0).astype(np.float64)).todense())
    err = np.abs(S - want)
    assert np.all(err <= (nterm + 1) * EPS * mag), float((err - (nterm + 1) * EPS * mag).max())
    return S, want


# ------------------------------------------------------------------ 1. against the reference, every column
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("similarity", SIMILARITIES)
def test_similarity_matches_the_reference_tie_aware(similarity, data):
    g = load_golden("itemknn_ref")
    dense = load_golden("itemknn_ref_dense_" + data)
    R = golden_matrix(g, data)
    I = R.shape[1]
    for shrink in (0, 10):
        pre = "%s_%s_s%d_" % (data, similarity, shrink)
        D = dense[pre + "dense"]
        bar = float(g[pre + "bar"])
        if similarity in ("adjusted", "pearson"):
            rel, atol = 0.0, 10 * bar                  # centred values are not integers: 10 x the reference's own bar
        else:
            rel, atol = REL_EXACT, 0.0
        for K in (5, 20):
            eng = _engine(R, K, shrink, similarity, **golden_params(g))
            W = eng.similarity()
            worst = check_columns(W, D, np.arange(I), K, rel, atol, pre + str(K))
            print("%s K=%d: engine vs fp64 columns %.3g; fp32 restatement vs fp64 (bar) %.3g; tolerance rel %.3g + %.3g"
                  % (pre, K, worst, bar, rel, atol))
            # per-column counts equal the reference's W_sparse (NaN entries of the reference aside: never stored here)
            Wr = sp.csr_matrix((g[pre + "w%d_data" % K], g[pre + "w%d_indices" % K], g[pre + "w%d_indptr" % K]),
                               shape=(I, I))
            Wr.data[np.isnan(Wr.data)] = 0
            Wr.eliminate_zeros()
            got_cnt, ref_cnt = np.diff(W.tocsc().indptr), np.diff(Wr.tocsc().indptr)
            print("%s K=%d: columns whose count differs from the reference's: %d"
                  % (pre, K, (got_cnt != ref_cnt).sum()))
            assert np.array_equal(got_cnt, ref_cnt), (pre, K, np.flatnonzero(got_cnt != ref_cnt))


# ------------------------------------------------------------------ 2. the engine's own tie rule
TIE_MATRIX = np.array([            # items 0, 1, 2 identical; 3, 4 identical; 5 alone; 6 = 5 + one user; 7 empty
    [1, 1, 1, 0, 0, 1, 1, 0],
    [1, 1, 1, 1, 1, 0, 0, 0],
    [0, 0, 0, 1, 1, 1, 1, 0],
    [1, 1, 1, 0, 0, 0, 1, 0],
    [0, 0, 0, 1, 1, 0, 0, 0],
    [0, 0, 0, 0, 0, 1, 1, 0]], dtype=np.float64)


@pytest.mark.parametrize("similarity", ["cosine", "jaccard", "dice", "euclidean"])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 100])
def test_own_tie_rule_larger_value_then_lower_index(K, similarity):
    R = sp.csr_matrix(TIE_MATRIX)
    I = R.shape[1]
    D = np.nan_to_num(dense_f64(R, similarity, 0), nan=0.0)
    vals = np.unique(D)
    assert np.all(np.diff(vals) > 1e-5 * np.abs(vals[1:])), "float64 values are equal or well apart"
    assert any(len(np.unique(D[:, i][D[:, i] != 0])) < np.count_nonzero(D[:, i]) for i in range(I)), "ties exist"
    W = _engine(R, K, 0, similarity).similarity().toarray()
    want = np.zeros((I, I))
    for i in range(I):
        order = np.lexsort((np.arange(I), -D[:, i]))[:min(K, I)]          # stable on (-value, index)
        want[order, i] = D[order, i]
    assert np.array_equal(W != 0, want != 0)
    assert np.all(np.abs(W - want) <= REL_EXACT * np.abs(want))


# ------------------------------------------------------------------ 3. scoring
def test_scores_match_r_times_w_and_the_reference_ratings():
    g = load_golden("itemknn_ref")
    pre, K = g["tie_free_case"]
    K = int(K)
    data, sim, shrink = re.fullmatch(r"(bin|rated)_(\w+)_s(\d+)_", str(pre)).groups()
    R = golden_matrix(g, data)
    eng = _engine(R, K, int(shrink), sim, **golden_params(g))
    users = g["ratings_users"]
    S, want = check_scores(eng, R, users)
    ref = g[pre + "ratings%d" % K]
    bar = float(g[pre + "bar_ratings%d" % K])
    W64 = sp.csr_matrix(eng.similarity(), dtype=np.float64)
    Ru = sp.csr_matrix(R, dtype=np.float64)[users]
    bound = (np.asarray(((Ru != 0).astype(np.float64) @ (W64 != 0).astype(np.float64)).todense()) + 1) * EPS * \
        np.asarray((abs(Ru) @ abs(W64)).todense())
    err = np.abs(S - ref)
    print("%s K=%d: scores vs the reference's ratings %.3g; fp32 restatement vs reference (bar) %.3g"
          % (pre, K, err.max(), bar))
    assert np.all(err <= 10 * bar + bound)
    # every user, another similarity with ties everywhere: still R @ W_engine
    eng = _engine(golden_matrix(g, "bin"), 20, 0, "jaccard")
    check_scores(eng, golden_matrix(g, "bin"), np.arange(R.shape[0]))


# ------------------------------------------------------------------ 4. shapes that reach every path
def _hub_graph(n_users=5300, n_items=1200, seed=11, rated=False, base_deg=0.15):
    """a hub item of ~5,100 users, a heavy user of 1,100 items (past 1,024: several strides of the workgroup), isolated
    users (u % 97 == 3) and isolated items (the last 9)"""
    rs = np.random.RandomState(seed)
    rows, cols = [], []
    for u in range(n_users):
        if u % 97 == 3:
            continue
        deg = int(min(60, max(1, rs.geometric(base_deg))))
        its = rs.choice(n_items - 10, deg, replace=False) + 1
        rows += [u] * deg
        cols += its.tolist()
    hub = [u for u in range(n_users) if u % 97 != 3][:5100]
    rows += hub
    cols += [0] * len(hub)
    rows += [7] * 1100
    cols += (np.arange(1100) + 1).tolist()
    R = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n_users, n_items))
    R.sum_duplicates()
    R.data[:] = rs.randint(1, 6, R.nnz) if rated else 1.0
    return R


def _cosine_family_f32(R, similarity, shrink):
    """cosine / pearson with every array and every operation in float32, the Gram as the reference takes it: a sparse
    product, whose sums run term by term in the arrays' own type.  Its gap to dense_f64 is the reference's float32
    rounding bar on this graph (the role of the recorded `bar` of the golden cases)."""
    f = np.float32
    M = sp.csr_matrix(R, dtype=f, copy=True)
    if similarity == "pearson":
        n = np.bincount(M.indices, minlength=M.shape[1])
        s = np.asarray(M.sum(axis=0), dtype=f).ravel()
        mean = np.zeros_like(s)
        mean[n > 0] = s[n > 0] / n[n > 0].astype(f)
        M.data -= mean[M.indices]
    C = np.asarray((M.T.tocsr() @ M).todense(), dtype=f)
    assert C.dtype == f
    s = np.sqrt(np.asarray(M.multiply(M).sum(axis=0), dtype=f).ravel().astype(f))
    np.fill_diagonal(C, 0)
    W = C * (f(1) / (s[None, :] * s[:, None] + f(shrink) + f(1e-6)))
    assert W.dtype == f
    return W


_HUB = {}


def hub_graph(rated):
    if rated not in _HUB:
        _HUB[rated] = _hub_graph(rated=rated)
    return _HUB[rated]


@pytest.mark.parametrize("similarity,rated,K,block", [
    ("cosine", True, 100, None), ("jaccard", False, 1, 500), ("jaccard", False, 800, 7 * 64 + 1),
    ("tversky", False, 5, None), ("euclidean", True, 5, 1000), ("pearson", True, 100, None),
    ("asymmetric", True, 5, None)])
def test_hub_graph_column_in_lds(similarity, rated, K, block):
    R = hub_graph(rated)
    U, I = R.shape
    assert np.diff(R.tocsc().indptr).max() >= 5000 and np.diff(R.indptr).max() > 1024
    assert (np.diff(R.indptr) == 0).sum() > 10 and (np.diff(R.tocsc().indptr) == 0).sum() >= 2
    assert block is None or I % block != 0
    params = dict(asymmetric_alpha=0.3, tversky_alpha=0.5, tversky_beta=1.0)
    eng = _engine(R, K, 2, similarity, block_cols=block, **params)
    W = eng.similarity()
    D = dense_f64(R, similarity, 2, **params)
    if similarity == "pearson":
        # centred values are not integers: 10 x the gap of a float32 restatement to the float64 columns, as in test 1
        bar = float(np.abs(_cosine_family_f32(R, similarity, 2).astype(np.float64) - D).max())
        rel, atol = 0.0, 10 * bar
        print("%s K=%d: fp32 restatement vs fp64 (bar) %.3g; tolerance %.3g" % (similarity, K, bar, atol))
    else:
        rel, atol = REL_EXACT, 0.0
    worst = check_columns(W, D, np.arange(I), K, rel, atol, similarity)
    print("%s K=%d: engine vs fp64 restatement %.3g" % (similarity, K, worst))
    users = np.concatenate([[3, 7, 100], np.arange(0, U, 211)])                 # isolated, heavy, ordinary
    S, _ = check_scores(eng, R, users, W)
    assert np.all(S[0] == 0)
    Wt = eng.scoring_csr()                                                     # the row form the scoring walks
    assert Wt.has_sorted_indices and (Wt - W).nnz == 0 and Wt.nnz == W.nnz
    assert np.all(np.diff(W.tocsc().indptr)[-9:] == 0)                         # the isolated items have no neighbours


def test_past_the_lds_bound_the_global_slab_form():
    """I = 12,300 > NRHIP_ITEMKNN_LDS_ITEMS: the accumulator column lives in the slab; 5,000 columns per launch does
    not divide I.  Few users, sparse: checked on a sample of columns (hub, ordinary, isolated) and of users."""
    from neurec_amd.itemknn import LDS_ITEMS
    R = _hub_graph(n_users=700, n_items=LDS_ITEMS + 12, seed=5, rated=True, base_deg=0.08)
    U, I = R.shape
    assert I > LDS_ITEMS and I % 5000 != 0
    cols = np.unique(np.concatenate([[0, 1, 2, I - 1, I - 2, 4999, 5000, 9999, 10000], np.arange(5, I, 97)]))
    for similarity, K in (("cosine", 5), ("euclidean", 20), ("dice", 100)):
        eng = _engine(R, K, 1, similarity, block_cols=5000)
        W = eng.similarity()
        D = dense_f64(R, similarity, 1, cols=cols)
        worst = check_columns(W, D, cols, K, REL_EXACT, 0.0, similarity)
        print("%s K=%d (global slab): engine vs fp64 restatement %.3g" % (similarity, K, worst))
        assert np.all(np.isfinite(W.data)) and np.all(W.data != 0)
        check_scores(eng, R, np.concatenate([[3, 7], np.arange(0, U, 53)]), W)


def test_euclidean_with_empty_items_has_no_nan_or_inf():
    R = sp.csr_matrix(TIE_MATRIX[:, [0, 3, 5, 7, 7, 6]])                        # items 3 and 4 are empty
    for K in (1, 3, 100):
        eng = _engine(R, K, 0, "euclidean")
        W = eng.similarity()
        assert np.all(np.isfinite(W.data)) and np.all(W.data != 0)
        assert W[[3, 4]].nnz == 0 and W[:, [3, 4]].nnz == 0
        S = eng.score(np.arange(R.shape[0], dtype=np.int32)).cpu().numpy()
        assert np.all(np.isfinite(S))
        check_columns(W, dense_f64(R, "euclidean", 0), np.arange(6), K, REL_EXACT, 0.0)


# ------------------------------------------------------------------ 5. determinism
def test_two_engines_and_two_score_calls_are_bit_identical():
    import torch
    R = hub_graph(True)
    a, b = (_engine(R, 100, 0, "cosine") for _ in range(2))
    for name in ("w_idx", "w_val", "w_cnt", "t_indptr", "t_cols", "t_vals"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    users = np.arange(0, R.shape[0], 7, dtype=np.int32)
    s1, s2 = a.score(users).clone(), a.score(users).clone()
    assert torch.equal(s1, s2) and torch.equal(s1, b.score(users))


# ------------------------------------------------------------------ 6. drop-in
ITEMKNN_PROPERTIES = """[hyperparameters]
neighbor = 5
shrink = 0
similarity = euclidean
asymmetric_alpha = 1
tversky_alpha = 0.5
tversky_beta = 0.5
verbose=1
"""
RESULT_LINE = re.compile(r"((?:\d\.\d{8}\s*\t){9}\d\.\d{8})\s*$")


def _write_dataset(root, n_users=120, n_items=90, seed=3):
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "dataset"), exist_ok=True)
    with open(os.path.join(root, "dataset", "toy.rating"), "w") as f:
        for u in range(n_users):
            liked = (u % 6) * 15 + rng.choice(15, 10, replace=False)       # 6 taste clusters
            for it in liked:
                f.write("%d\t%d\t%d\t%d\n" % (u + 7, it + 300, 5, rng.randint(1, 10**6)))


def _run(tmp_path, argv):
    from neurec_amd.main import main
    path = defaults.write_default_configs(str(tmp_path), overrides={
        "data.input.path": os.path.join(str(tmp_path), "dataset"), "data.input.dataset": "toy",
        "test_batch_size": "64"})
    with open(os.path.join(str(tmp_path), "conf", "ItemKNN.properties"), "w") as f:
        f.write(ITEMKNN_PROPERTIES)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return main(argv=argv, properties=path)
    finally:
        os.chdir(cwd)


def _log_text(tmp_path):
    folder = os.path.join(str(tmp_path), "log", "toy", "ItemKNN")
    files = os.listdir(folder)
    assert len(files) == 1 and files[0].startswith("toy_ItemKNN_")
    with open(os.path.join(folder, files[0])) as f:
        return f.read()


def test_itemknn_config_drops_in_and_recommends(tmp_path):
    import torch
    _write_dataset(str(tmp_path))
    model = _run(tmp_path, ["--recommender=ItemKNN", "--similarity=cosine", "--neighbor=10"])
    text = _log_text(tmp_path)
    assert "ItemKNN's hyperparameters:" in text
    assert len(re.findall(r"metrics:\tPrecision@10", text)) == 1
    results = [m.group(1) for m in (RESULT_LINE.search(ln) for ln in text.splitlines()) if m]
    assert len(results) == 1 and text.index("metrics:\t") < text.index(results[0])
    ndcg = float(results[0].split("\t")[4])                                   # NDCG@10 is the 5th number
    uni = model.evaluator.evaluator
    users = list(uni.user_pos_test.keys())
    assert uni._format(uni._evaluate_scores(model, users)).strip() == results[0].strip()

    class Zero:
        def predict(self, user_ids, items=None):
            return torch.zeros((len(user_ids), model.num_items), dtype=torch.float32, device="cuda")
    ndcg0 = float(uni._format(uni._evaluate_scores(Zero(), users)).split("\t")[4])
    print("NDCG@10: all-zero scores %.4f, ItemKNN cosine K=10 %.4f" % (ndcg0, ndcg))
    assert ndcg > 0.3 and ndcg > ndcg0 + 0.15
    # predict contract: a [B, I] device tensor; candidate mode -> per-user arrays, slices of the same rows
    full = model.predict([0, 5, 9], None)
    assert isinstance(full, torch.Tensor) and full.is_cuda and tuple(full.shape) == (3, model.num_items)
    assert full.dtype == torch.float32
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    host = full.cpu().numpy()
    assert [len(c) for c in cand] == [3, 1]
    assert np.array_equal(cand[0], host[0][[1, 2, 3]]) and np.array_equal(cand[1], host[1][[7]])


def test_the_shipped_default_runs_to_a_result_line(tmp_path):
    _write_dataset(str(tmp_path))
    model = _run(tmp_path, ["--recommender=ItemKNN"])
    assert model.similarity == "euclidean" and model.topK == 5
    results = [ln for ln in _log_text(tmp_path).splitlines() if RESULT_LINE.search(ln)]
    assert len(results) == 1


# ------------------------------------------------------------------ 7. refusals
def test_refusals(tmp_path):
    R = sp.csr_matrix(np.eye(6, 5))
    with pytest.raises(ValueError, match="value for parameter 'mode' not recognized"):
        _engine(R, 5, 0, "manhattan")
    with pytest.raises(ValueError, match="neighbor"):
        _engine(R, 0, 0, "cosine")
    with pytest.raises(NotImplementedError, match="1024"):
        _engine(R, 1025, 0, "cosine")
    _write_dataset(str(tmp_path))
    with pytest.raises(ValueError):
        _run(tmp_path, ["--recommender=ItemKNN", "--neighbor=0"])
