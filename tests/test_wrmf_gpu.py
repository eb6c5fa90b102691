"""WRMF on the GPU: the batched half-sweeps (csrc/wrmf.hip through neurec_amd/wrmf.py) against the reference class's own
trace and an fp64 ALS, bit-for-bit determinism, the drop-in run through neurec_amd.main, and the refusals."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_golden
from neurec_amd import defaults

pytestmark = pytest.mark.gpu


def als_half(R, Y, alpha, lam):
    """fp64: x_u = (Y^T Y + alpha sum_{j in N(u)} y_j y_j^T + lam I)^{-1} (1 + alpha) sum_{j in N(u)} y_j"""
    Y = np.asarray(Y, np.float64)
    d = Y.shape[1]
    G = Y.T @ Y
    X = np.zeros((R.shape[0], d))
    for u in range(R.shape[0]):
        nb = R.indices[R.indptr[u]:R.indptr[u + 1]]
        if len(nb):
            Yn = Y[nb]
            X[u] = np.linalg.solve(G + alpha * (Yn.T @ Yn) + lam * np.eye(d), (1 + alpha) * Yn.sum(axis=0))
    return X


def _engine(P0, Q0, R, alpha, reg):
    from neurec_amd.wrmf import WRMFEngine
    return WRMFEngine(P0, Q0, R, alpha, reg)


def test_matches_the_reference_class_trace():
    """Two epochs from the trace's Q0 (and a user table unlike its P0: the first half-sweep overwrites it).  The bound
    is the trace's own fp32-vs-fp64 gap `bar` (the reference's fp32 LU solves against their fp64 twin) times 10: the
    engine rounds differently in every stage (Gram and neighbour sums in another order, an L D L^T factorisation
    instead of LU), each stage an fp32 error of the same order as the reference's own."""
    import torch
    g = load_golden("tfgraph_wrmf")
    U, I = (int(x) for x in g["shape"])
    R = sp.csr_matrix((np.ones(len(g["indices"]), np.float32), g["indices"], g["indptr"]), shape=(U, I))
    P0 = np.random.RandomState(5).uniform(-1, 1, g["P0"].shape).astype(np.float32)
    eng = _engine(P0, g["Q0"], R, float(g["alpha"]), float(g["reg_mf"]))
    deg_u, deg_i = np.diff(R.indptr), np.diff(R.tocsc().indptr)
    for e in range(int(g["epochs"])):
        eng.epoch()
        P, Q = [t.cpu().numpy() for t in eng.tables()]
        for name, got, f64, f32, deg in (("P", P, g["f64_P"][e], g["f32_P"][e], deg_u),
                                         ("Q", Q, g["f64_Q"][e], g["f32_Q"][e], deg_i)):
            bar = np.abs(f32.astype(np.float64) - f64).max()
            err = np.abs(got.astype(np.float64) - f64).max()
            print("epoch %d %s: engine vs fp64 %.3g, reference fp32 vs fp64 (bar) %.3g" % (e + 1, name, err, bar))
            assert err <= 10 * bar, (e, name, err, bar)
            assert np.all(got[deg == 0] == 0)
        S = P[g["ratings_users"]].astype(np.float64) @ Q.T.astype(np.float64)
        assert np.abs(S - g["f64_ratings"][e]).max() <= 10 * np.abs(g["f32_ratings"][e] - g["f64_ratings"][e]).max() \
            + 1e-5 * np.abs(S).max()
    torch.cuda.synchronize()


def _hub_graph(n_users=5300, n_items=1200, seed=11):
    """power-law-ish pattern with a hub item of 5,100 users and a heavy user of 1,500 items (both past the
    1,024-long chunk: the chunked path runs on both sides), isolated users and items"""
    rs = np.random.RandomState(seed)
    rows, cols = [], []
    for u in range(n_users):
        if u % 97 == 3:
            continue                                        # isolated users
        deg = int(min(60, max(1, rs.geometric(0.15))))
        its = rs.choice(n_items - 10, deg, replace=False) + 1
        rows += [u] * deg
        cols += its.tolist()
    hub = [u for u in range(n_users) if u % 97 != 3][:5100]
    rows += hub
    cols += [0] * len(hub)
    heavy = 7
    rows += [heavy] * 1100
    cols += (np.arange(1100) + 1).tolist()                  # items n_items-9 .. n_items-1 stay isolated
    R = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_users, n_items))
    R.data[:] = 1.0
    R.sum_duplicates()
    R.data[:] = 1.0
    return R


@pytest.mark.parametrize("alpha", [1.0, 40.0])
@pytest.mark.parametrize("d", [1, 7, 16, 33, 64, 128])
def test_half_sweeps_match_fp64_als(d, alpha):
    """Each half-sweep against an fp64 numpy ALS of the same inputs (the item half from the engine's own user table):
    relative error (max |got - want| / max |want|) at most 1e-4, fp32 sums and an fp32 factorisation of matrices
    whose condition these shapes keep moderate."""
    R = _hub_graph()
    U, I = R.shape
    assert np.diff(R.tocsc().indptr).max() >= 5000 and np.diff(R.indptr).max() > 1024
    rs = np.random.RandomState(d)
    Q0 = rs.uniform(-0.5, 0.5, (I, d)).astype(np.float32)
    eng = _engine(np.zeros((U, d), np.float32), Q0, R, alpha, 0.1)
    assert eng.users.n_chunks > 0 and eng.items.n_chunks > 0
    Rt = R.T.tocsr()
    eng.solve_users()
    P = eng.P.cpu().numpy()
    want_P = als_half(R, Q0, alpha, 0.1)
    eng.solve_items()
    Q = eng.Q.cpu().numpy()
    want_Q = als_half(Rt, P, alpha, 0.1)
    for name, got, want, deg in (("P", P, want_P, np.diff(R.indptr)), ("Q", Q, want_Q, np.diff(Rt.indptr))):
        rel = np.abs(got - want).max() / np.abs(want).max()
        print("d=%d alpha=%g %s: relative error %.3g" % (d, alpha, name, rel))
        assert rel <= 1e-4, (d, alpha, name, rel)
        assert (deg == 0).any() and np.all(got[deg == 0] == 0)


def test_two_engines_give_bit_identical_tables():
    import torch
    R = _hub_graph()
    U, I = R.shape
    rs = np.random.RandomState(3)
    P0, Q0 = (rs.uniform(-0.5, 0.5, (n, 64)).astype(np.float32) for n in (U, I))
    out = []
    for _ in range(2):
        eng = _engine(P0, Q0, R, 10.0, 0.1)
        eng.epoch()
        eng.epoch()
        out.append([t.clone() for t in eng.tables()])
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ------------------------------------------------------------------ drop-in
WRMF_PROPERTIES = """[hyperparameters]
epochs=300
embedding_size=16
reg_mf=0.1
alpha=10
init_method=uniform
stddev=0.01
verbose=1
"""


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
    with open(os.path.join(str(tmp_path), "conf", "WRMF.properties"), "w") as f:
        f.write(WRMF_PROPERTIES)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return main(argv=argv, properties=path)
    finally:
        os.chdir(cwd)


def test_wrmf_config_drops_in_and_learns(tmp_path):
    import torch
    from neurec_amd.util.tool import get_initializer
    _write_dataset(str(tmp_path))
    np.random.seed(2018)
    model = _run(tmp_path, ["--recommender=WRMF", "--epochs=3", "--verbose=1"])
    folder = os.path.join(str(tmp_path), "log", "toy", "WRMF")
    files = os.listdir(folder)
    assert len(files) == 1 and files[0].startswith("toy_WRMF_")
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "WRMF's hyperparameters:" in text
    lines = [ln for ln in text.splitlines()
             if re.search(r"metrics:\t|iteration \d+ finished in [0-9.]+ seconds|epoch \d+:\t", ln)]
    kinds = [("m" if "metrics:" in ln else "i%s" % re.search(r"iteration (\d+)", ln).group(1)
              if "iteration" in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)) for ln in lines]
    assert kinds == ["m", "i1", "e1", "i2", "e2", "i3", "e3"], kinds
    assert "metrics:\tPrecision@10" in lines[0]
    evals = re.findall(r"epoch (\d+):\t(.+)", text)
    last = evals[-1][1].split("\t")
    assert len(last) == 10 and all(re.fullmatch(r"\d\.\d{8}\s*", x) for x in last)
    # factor path == score-matrix (plugin) path == the logged line, to the last printed digit
    uni = model.evaluator.evaluator
    users = list(uni.user_pos_test.keys())
    line_factor = uni._format(uni._evaluate_factors(model, users))
    line_scores = uni._format(uni._evaluate_scores(model, users))
    assert line_factor == line_scores
    assert line_factor.strip() == evals[-1][1].strip()
    ndcg = float(line_factor.split("\t")[4])                                  # NDCG@10 is the 5th number
    # the same evaluation on the initial random tables (the plugin's initializer, seed 2017)
    init = get_initializer("uniform", 0.01, seed=2017)
    P1, Q1 = model.engine.P, model.engine.Q
    model.engine.P = torch.from_numpy(init([model.num_users, 16])).cuda()
    model.engine.Q = torch.from_numpy(init([model.num_items, 16])).cuda()
    ndcg0 = float(uni._format(uni._evaluate_factors(model, users)).split("\t")[4])
    model.engine.P, model.engine.Q = P1, Q1
    print("NDCG@10: initial tables %.4f, after 3 epochs %.4f" % (ndcg0, ndcg))
    assert ndcg > 0.3 and ndcg > ndcg0 + 0.15
    # predict contract: [B, I] float32 array; candidate mode -> list of per-user arrays
    full = model.predict([0, 5, 9], None)
    assert full.shape == (3, model.num_items) and full.dtype == np.float32
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])
    P, Q = [t.cpu().numpy().astype(np.float64) for t in model.get_eval_factors()]
    assert np.abs(full - P[[0, 5, 9]] @ Q.T).max() <= 1e-5 * max(1.0, np.abs(full).max())


def test_refusals():
    R = sp.csr_matrix(np.eye(6, 5, dtype=np.float32))
    with pytest.raises(NotImplementedError, match="128"):
        _engine(np.zeros((6, 129), np.float32), np.zeros((5, 129), np.float32), R, 10.0, 0.1)
    with pytest.raises(ValueError, match="reg_mf"):
        _engine(np.zeros((6, 16), np.float32), np.zeros((5, 16), np.float32), R, 10.0, 0.0)


def test_plugin_refuses_what_the_engine_refuses(tmp_path):
    _write_dataset(str(tmp_path))
    with pytest.raises(NotImplementedError):
        _run(tmp_path, ["--recommender=WRMF", "--epochs=1", "--embedding_size=129"])
    with pytest.raises(ValueError):
        _run(tmp_path, ["--recommender=WRMF", "--epochs=1", "--reg_mf=0"])
