"""ItemKNN without a GPU: the golden files made from the reference's own classes (tests/golden/itemknn_ref*.npz), the
float64 restatement the GPU tests measure against pinned to the reference's recorded columns, the plugin lookup and the
C ABI surface of the new entries."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["nrhip_itemknn_workspace_bytes", "nrhip_itemknn_build", "nrhip_itemknn_score"]
SIMILARITIES = ["cosine", "adjusted", "asymmetric", "pearson", "jaccard", "dice", "tversky", "euclidean"]
DATA = ["bin", "rated"]


def dense_f64(R, similarity, shrink, asymmetric_alpha=0.5, tversky_alpha=1.0, tversky_beta=1.0, cols=None):
    """The reference's similarity columns in float64, restated (ItemKNN.py:412-504 and :89-181 with normalize=True):
    out[j, k] = W[j, cols[k]] before the top-K cut; euclidean pairs of two empty items are NaN, as there."""
    M = sp.csr_matrix(R, dtype=np.float64, copy=True)
    M.sum_duplicates()
    if similarity == "adjusted":
        n = np.diff(M.indptr)
        s = np.asarray(M.sum(axis=1)).ravel()
        mean = np.zeros_like(s)
        mean[n > 0] = s[n > 0] / n[n > 0]
        M.data -= np.repeat(mean, n)
    elif similarity == "pearson":
        n = np.bincount(M.indices, minlength=M.shape[1])
        s = np.asarray(M.sum(axis=0)).ravel()
        mean = np.zeros_like(s)
        mean[n > 0] = s[n > 0] / n[n > 0]
        M.data -= mean[M.indices]
    elif similarity in ("jaccard", "tanimoto", "dice", "tversky"):
        M.data[:] = 1.0
    I = M.shape[1]
    cols = np.arange(I) if cols is None else np.asarray(cols)
    Mc = M.tocsc()
    C = np.asarray((M.T @ Mc[:, cols]).todense())                    # [I, len(cols)]
    ssq = np.asarray(M.power(2).sum(axis=0)).ravel()
    own = (np.arange(I)[:, None] == cols[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        if similarity == "euclidean":
            s = np.sqrt(ssq)
            d2 = ssq[:, None] + ssq[cols][None, :] - 2 * C
            d2[own] = 0.0
            W = 1 / (np.sqrt(d2 / (s[cols][None, :] * s[:, None])) + shrink + 1e-9)
        else:
            C[own] = 0.0
            if similarity in ("jaccard", "tanimoto"):
                den = ssq[cols][None, :] + ssq[:, None] - C + shrink + 1e-6
            elif similarity == "dice":
                den = ssq[cols][None, :] + ssq[:, None] + shrink + 1e-6
            elif similarity == "tversky":
                den = C + (ssq[cols][None, :] - C) * tversky_alpha + (ssq[:, None] - C) * tversky_beta + shrink + 1e-6
            elif similarity == "asymmetric":
                s = np.sqrt(ssq)
                den = np.power(s, 2 * asymmetric_alpha)[cols][None, :] * \
                    np.power(s, 2 * (1 - asymmetric_alpha))[:, None] + shrink + 1e-6
            elif similarity in ("cosine", "adjusted", "pearson"):
                s = np.sqrt(ssq)
                den = s[cols][None, :] * s[:, None] + shrink + 1e-6
            else:
                raise ValueError(similarity)
            W = C * (1 / den)
    W[own] = 0.0
    return W


def golden_matrix(g, data):
    U, I = (int(x) for x in g["shape"])
    return sp.csr_matrix((g[data + "_data"], g[data + "_indices"], g[data + "_indptr"]), shape=(U, I))


def golden_params(g):
    return dict(asymmetric_alpha=float(g["asymmetric_alpha"]), tversky_alpha=float(g["tversky_alpha"]),
                tversky_beta=float(g["tversky_beta"]))


def test_golden_files_hold_the_recorded_keys():
    g = load_golden("itemknn_ref")
    U, I = (int(x) for x in g["shape"])
    assert (U, I) == (157, 131) and list(g["similarities"]) == SIMILARITIES
    assert list(g["shrinks"]) == [0, 10] and list(g["neighbors"]) == [5, 20]
    users = g["ratings_users"]
    assert np.array_equal(users, np.arange(0, U, 15))
    for data in DATA:
        dense = load_golden("itemknn_ref_dense_" + data)
        R = golden_matrix(g, data)
        assert R.nnz > 0 and (set(np.unique(R.data)) == {1.0} if data == "bin" else R.data.max() == 5.0)
        for sim in SIMILARITIES:
            for shrink in (0, 10):
                pre = "%s_%s_s%d_" % (data, sim, shrink)
                assert dense[pre + "dense"].shape == (I, I) and dense[pre + "dense"].dtype == np.float64
                assert g[pre + "bar"] >= 0
                for K in (5, 20):
                    W = sp.csr_matrix((g[pre + "w%d_data" % K], g[pre + "w%d_indices" % K], g[pre + "w%d_indptr" % K]),
                                      shape=(I, I))
                    assert W.data.dtype == np.float32 and np.diff(W.tocsc().indptr).max() <= K
                    assert g[pre + "ratings%d" % K].shape == (len(users), I) and g[pre + "bar_ratings%d" % K] >= 0
    pre, K = g["tie_free_case"]
    assert pre.startswith("rated_") and g[pre + "w%s_data" % K].size > 0


def test_tie_free_case_has_no_boundary_tie_and_ties_are_the_rule_elsewhere():
    g = load_golden("itemknn_ref")
    pre, K = g["tie_free_case"]
    K = int(K)

    def boundary_ties(dense, K, rel):
        v = -np.sort(-np.nan_to_num(dense, nan=0.0), axis=0)
        a, b = v[K - 1], v[K]
        return int(np.sum((np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b))) & ~((a == 0) & (b == 0))))

    assert boundary_ties(load_golden("itemknn_ref_dense_rated")[pre + "dense"], K, 1e-4) == 0
    assert boundary_ties(load_golden("itemknn_ref_dense_bin")["bin_jaccard_s0_dense"], 5, 0.0) >= 20


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("similarity", SIMILARITIES)
def test_float64_restatement_reproduces_the_reference_columns(similarity, data):
    """dense_f64 — the yardstick of the GPU tests on graphs the reference's Python loop is too slow for — against the
    columns the reference's own classes produced: 1e-12 relative to max(1, |value|), NaN in the same places."""
    g = load_golden("itemknn_ref")
    dense = load_golden("itemknn_ref_dense_" + data)
    R = golden_matrix(g, data)
    for shrink in (0, 10):
        want = dense["%s_%s_s%d_dense" % (data, similarity, shrink)]
        got = dense_f64(R, similarity, shrink, **golden_params(g))
        assert np.array_equal(np.isnan(got), np.isnan(want))
        if similarity == "euclidean":
            assert np.isnan(want).sum() == 2             # the pair of the two empty items, both ways
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= 1e-12 * np.maximum(1.0, np.abs(want[ok])))
        # the same columns through the `cols` argument
        cols = np.array([0, 7, 130])
        sub = dense_f64(R, similarity, shrink, cols=cols, **golden_params(g))
        assert np.array_equal(np.nan_to_num(sub), np.nan_to_num(got[:, cols]))


def test_reference_w_sparse_is_a_top_k_of_its_columns():
    """W_sparse (float32) holds, per column, values equal to the K largest of the recorded float64 column, cast."""
    g = load_golden("itemknn_ref")
    I = int(g["shape"][1])
    for data in DATA:
        dense = load_golden("itemknn_ref_dense_" + data)
        for sim in SIMILARITIES:
            pre = "%s_%s_s0_" % (data, sim)
            D = np.nan_to_num(dense[pre + "dense"], nan=0.0)
            for K in (5, 20):
                W = sp.csr_matrix((g[pre + "w%d_data" % K], g[pre + "w%d_indices" % K], g[pre + "w%d_indptr" % K]),
                                  shape=(I, I)).tocsc()
                for i in range(I):
                    got = np.sort(W.data[W.indptr[i]:W.indptr[i + 1]])[::-1]
                    got = got[~np.isnan(got)]
                    top = -np.sort(-D[:, i])[:K]
                    want = top[top != 0].astype(np.float32)
                    assert np.array_equal(got[:len(want)], want[:len(got)]) and abs(len(got) - len(want)) <= 1, (pre, K, i)


def test_find_recommender_resolves_itemknn():
    from neurec_amd.main import find_recommender
    cls = find_recommender("ItemKNN")
    assert cls.__name__ == "ItemKNN" and cls.__module__ == "neurec_amd.model.general_recommender.ItemKNN"


def test_header_declares_and_binding_covers_the_itemknn_entries():
    with open(os.path.join(ROOT, "include", "neurec_hip.h")) as f:
        text = f.read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, text), name
    assert "#define NRHIP_ITEMKNN_LDS_ITEMS 12288" in text and "#define NRHIP_ITEMKNN_MAX_NEIGHBOR 1024" in text
    assert "ItemKNN.py:395-547" in text and "ItemKNN.py:60-214" in text and "ItemKNN.py:573" in text
    assert "TIE RULE" in text
    from neurec_amd import _lib, itemknn
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)
    assert (itemknn.LDS_ITEMS, itemknn.MAX_NEIGHBOR) == (12288, 1024)


def test_workspace_query_and_refusals():
    import ctypes as C
    from neurec_amd import _lib
    b = C.c_size_t(0)
    _lib.call("nrhip_itemknn_workspace_bytes", 1200, 100, 1200, C.byref(b))
    assert b.value == 1200 * 100 * 8                                  # column in LDS: the transpose's keys only
    _lib.call("nrhip_itemknn_workspace_bytes", 12289, 5, 1000, C.byref(b))
    assert b.value >= 1000 * 12289 * 4 + 12289 * 5 * 8                # past the LDS bound: + the [block][I] slab
    with pytest.raises(NotImplementedError, match="1024"):
        _lib.call("nrhip_itemknn_workspace_bytes", 100, 1025, 10, C.byref(b))
    with pytest.raises(ValueError, match="neighbor"):
        _lib.call("nrhip_itemknn_workspace_bytes", 100, 0, 10, C.byref(b))


def test_host_side_refusals_need_no_gpu():
    from neurec_amd.itemknn import similarity_inputs
    R = sp.csr_matrix(np.eye(4, 5))
    with pytest.raises(ValueError, match="value for parameter 'mode' not recognized"):
        similarity_inputs(R, "manhattan")
    M, v, na, nb = similarity_inputs(sp.csr_matrix(np.array([[1., 3.], [5., 0.]])), "adjusted")
    assert np.allclose(v, [-1, 1, 0]) and np.allclose(na, np.sqrt([1, 1]))
