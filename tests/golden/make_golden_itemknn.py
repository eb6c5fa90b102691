"""Golden ItemKNN results produced by the REFERENCE's own classes (model/general_recommender/ItemKNN.py).

The module is imported whole and unchanged through oracle/ref_models.py, as make_golden_wrmf.py does for WRMF; it
needs no TensorFlow call.  For every similarity name x shrink in {0, 10} x the toy matrix as stored (all ratings 1,
`bin`) and with integer ratings 1..5 from a fixed seed (`rated`), all fed as float64 like the reference's own Dataset
does, the file records under the prefix `<data>_<similarity>_s<shrink>_`:

    dense       (in itemknn_ref_dense_<data>.npz, one file per matrix: the columns are most of the bytes)
                the reference's full similarity columns, float64 [I, I] (dense[j, i] = W[j, i]):
                Compute_Similarity(..., topK=I).compute_similarity() with the module's final
                `sps.csr_matrix(..., dtype=np.float32)` cast held at float64 (the one name patched: `sps`, for that call)
    w5_* / w20_*        the ItemKNN class's W_sparse for neighbor = 5 / 20 (CSR arrays, float32 as the reference casts)
    ratings5 / ratings20    its `ratings` rows (float64) for the users `ratings_users` (every 15th)
    bar         max |f32 - dense| of a float32 numpy restatement of the same formulas (Gram, formula, all in float32):
                the reference's own fp32 rounding bar, the role f32_* against f64_* plays in tfgraph_wrmf.npz
    bar_ratings5 / bar_ratings20    the same gap for the ratings rows (float32 R @ top-K of the float32 columns)
                (the restatement itself is f32_columns() below; only its gaps are stored)

`tie_free_case` names one recorded (prefix, K) in which no column's K-th and (K+1)-th largest values lie within 1e-4
relative of each other (pairs of exact zeros aside: zeros are never stored) — the only case a test may compare with the
reference's `ratings` directly.  Euclidean: the pair of the toy matrix's two empty items is NaN in `dense` (0/0).

    python tests/golden/make_golden_itemknn.py              # needs the reference tree
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_models as rm          # noqa: E402
from make_golden_tfgraph import toy_matrix    # noqa: E402

SIMILARITIES = ["cosine", "adjusted", "asymmetric", "pearson", "jaccard", "dice", "tversky", "euclidean"]
SHRINKS = [0, 10]
NEIGHBORS = [5, 20]
PARAMS = dict(asymmetric_alpha=0.3, tversky_alpha=0.5, tversky_beta=1.0)


def matrices():
    R = toy_matrix().astype(np.float64)
    rated = R.copy()
    rated.data[:] = np.random.RandomState(4242).randint(1, 6, len(rated.data)).astype(np.float64)
    return {"bin": R, "rated": rated}


def f32_columns(R, similarity, shrink):
    """the same formulas with every array and every operation in float32 (ItemKNN.py:412-504, 89-181)"""
    f = np.float32
    M = sp.csr_matrix(R, dtype=f, copy=True)
    if similarity == "adjusted":
        n = np.diff(M.indptr)
        s = np.asarray(M.sum(axis=1), dtype=f).ravel()
        mean = np.zeros_like(s)
        mean[n > 0] = s[n > 0] / n[n > 0].astype(f)
        M.data -= np.repeat(mean, n)
    elif similarity == "pearson":
        n = np.bincount(M.indices, minlength=M.shape[1])
        s = np.asarray(M.sum(axis=0), dtype=f).ravel()
        mean = np.zeros_like(s)
        mean[n > 0] = s[n > 0] / n[n > 0].astype(f)
        M.data -= mean[M.indices]
    elif similarity in ("jaccard", "dice", "tversky"):
        M.data[:] = 1
    D = M.toarray()
    C = (D.T @ D).astype(f)
    ssq = (D * D).sum(axis=0, dtype=f)
    shrink, eps6, eps9 = f(shrink), f(1e-6), f(1e-9)
    with np.errstate(divide="ignore", invalid="ignore"):
        if similarity == "euclidean":
            s = np.sqrt(ssq)
            d2 = ssq[:, None] + ssq[None, :] - f(2) * C
            np.fill_diagonal(d2, 0)
            W = f(1) / (np.sqrt(d2 / (s[:, None] * s[None, :])) + shrink + eps9)
        else:
            np.fill_diagonal(C, 0)
            if similarity in ("cosine", "adjusted", "pearson"):
                s = np.sqrt(ssq)
                W = C * (f(1) / (s[None, :] * s[:, None] + shrink + eps6))
            elif similarity == "asymmetric":
                s = np.sqrt(ssq)
                a = np.power(s, f(2 * PARAMS["asymmetric_alpha"]))
                b = np.power(s, f(2 * (1 - PARAMS["asymmetric_alpha"])))
                W = C * (f(1) / (a[None, :] * b[:, None] + shrink + eps6))      # W[j, i]: a of column i, b of row j
            elif similarity == "jaccard":
                W = C * (f(1) / (ssq[None, :] + ssq[:, None] - C + shrink + eps6))
            elif similarity == "dice":
                W = C * (f(1) / (ssq[None, :] + ssq[:, None] + shrink + eps6))
            else:
                ta, tb = f(PARAMS["tversky_alpha"]), f(PARAMS["tversky_beta"])
                W = C * (f(1) / (C + (ssq[None, :] - C) * ta + (ssq[:, None] - C) * tb + shrink + eps6))
    np.fill_diagonal(W, 0)
    return W.astype(f)


def topk_dense(W, K):
    """columns cut to their K largest (value descending, index ascending among equals), zeros / NaN dropped"""
    out = np.zeros_like(W)
    for i in range(W.shape[1]):
        col = np.nan_to_num(W[:, i], nan=0.0)
        order = np.lexsort((np.arange(len(col)), -col))[:K]
        out[order, i] = col[order]
    return out


class _Float64Sparse:
    """scipy.sparse as the reference module sees it while the dense columns are taken: csr_matrix without the
    float32 cast"""

    def __getattr__(self, name):
        return getattr(sp, name)

    @staticmethod
    def csr_matrix(*args, **kwargs):
        kwargs.pop("dtype", None)
        return sp.csr_matrix(*args, dtype=np.float64, **kwargs)


def dense_columns(mod, R, similarity, shrink):
    saved = mod.sps
    mod.sps = _Float64Sparse()
    try:
        with np.errstate(divide="ignore", invalid="ignore"):
            W = mod.Compute_Similarity(R.tocsc(), shrink=shrink, topK=R.shape[1], normalize=True,
                                       similarity=similarity, **PARAMS).compute_similarity()
    finally:
        mod.sps = saved
    assert W.dtype == np.float64
    return W.toarray()


def has_boundary_tie(dense, K, rel=1e-4):
    v = -np.sort(-np.nan_to_num(dense, nan=0.0), axis=0)
    a, b = v[K - 1], v[K]
    return bool(np.any((np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b))) & ~((a == 0) & (b == 0))))


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    out, tie_free = {}, []
    mats = matrices()
    dense_out = {data: {} for data in mats}
    U, I = mats["bin"].shape
    users = np.arange(0, U, 15, dtype=np.int32)
    rm.RecordingEvaluator.users = users.tolist()
    mod = rm.load("ItemKNN")
    for data, R in mats.items():
        out["%s_indptr" % data] = R.indptr.astype(np.int64)
        out["%s_indices" % data] = R.indices.astype(np.int32)
        out["%s_data" % data] = R.data.astype(np.float64)
        for sim in SIMILARITIES:
            for shrink in SHRINKS:
                pre = "%s_%s_s%d_" % (data, sim, shrink)
                dense = dense_columns(mod, R, sim, shrink)
                f32 = f32_columns(R, sim, shrink)
                dense_out[data][pre + "dense"] = dense
                out[pre + "bar"] = np.float64(np.abs(np.nan_to_num(f32, nan=0.0).astype(np.float64)
                                                     - np.nan_to_num(dense, nan=0.0)).max())
                for K in NEIGHBORS:
                    hyper = dict(neighbor=K, shrink=shrink, similarity=sim, verbose=1, **PARAMS)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        model, _, _ = rm.build("ItemKNN", rm.Dataset(R), hyper, "float64")
                    W = model.W_sparse.tocsr()
                    W.sort_indices()
                    out[pre + "w%d_data" % K] = W.data.astype(np.float32)
                    out[pre + "w%d_indices" % K] = W.indices.astype(np.int32)
                    out[pre + "w%d_indptr" % K] = W.indptr.astype(np.int64)
                    ratings = np.asarray(model.predict(users.tolist(), None), np.float64)
                    out[pre + "ratings%d" % K] = ratings
                    r32 = R.astype(np.float32)[users].toarray() @ topk_dense(f32, K)
                    out[pre + "bar_ratings%d" % K] = np.float64(np.abs(np.nan_to_num(r32.astype(np.float64))
                                                                       - np.nan_to_num(ratings)).max())
                    if not has_boundary_tie(dense, K):
                        tie_free.append((pre, K))
    # the tie-free case the tests compare with `ratings` directly: on the rated matrix (on the binary one `adjusted`
    # and `pearson` are all zero), pearson with K = 5 first, shrink 0 when it qualifies
    prefer = [("rated_pearson_s0_", 5), ("rated_pearson_s10_", 5), ("rated_adjusted_s0_", 5), ("rated_cosine_s0_", 5)]
    chosen = [c for c in prefer if c in tie_free]
    assert chosen, "none of %s is free of ties at the K-th place: choose another seed or K" % (prefer,)
    pre, K = chosen[0]
    out["tie_free_case"] = np.asarray([pre, str(K)])
    out["tie_free_all"] = np.asarray(["%s%d" % c for c in tie_free])
    out["ratings_users"] = users
    out["shape"] = np.asarray([U, I], np.int64)
    out["similarities"] = np.asarray(SIMILARITIES)
    out["shrinks"] = np.asarray(SHRINKS, np.int64)
    out["neighbors"] = np.asarray(NEIGHBORS, np.int64)
    for k, v in PARAMS.items():
        out[k] = np.float64(v)
    sizes = []
    for name, arrays in [("itemknn_ref", out)] + [("itemknn_ref_dense_" + d, a) for d, a in dense_out.items()]:
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        sizes.append("%s %d bytes" % (name, os.path.getsize(path)))
    print("wrote %s; tie-free case %s K=%d (of %d tie-free)" % (", ".join(sizes), pre, K, len(tie_free)))


if __name__ == "__main__":
    main()
