"""CFGAN on the GPU (csrc/cfgan.hip through neurec_amd/cfgan.py): the reference class's recorded runs replayed with its
own masks (tests/golden/tfgraph_cfgan.npz) — every variable after every step, the loss terms, the ratings in both modes;
the mask builder against its CPU restatement, bit for bit; both steps on the edge shapes against the float64
restatement, which test_cfgan_cpu.py holds to the same trace and to autograd; determinism, clean gradient buffers, the
refusals, empty work, and the drop-in run through neurec_amd.main in a child process.

The tolerance is the project's rule (`_close` of test_gru4rec_gpu.py): 4 x the float32 reference's own distance from the
float64 one for that tensor and step, plus 1e-5 max|want|.  For the trace the distance is the reference's, read from the
golden; where the trace holds none (the loss terms, the edge shapes) it is the restatement's float32 run's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import cfgan_restatement as P
from test_cfgan_cpu import restated
from test_gru4rec_gpu import _close

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "tfgraph_cfgan.npz"))


def _engine(tables, R_users_items, hg, hd, mode="userBased", reg_g=0.001, reg_d=0.0, opt_g="adam", opt_d="adam",
            batch=16, zr_ratio=P.ZR_RATIO, zp_ratio=P.ZP_RATIO, lr_g=P.LR_G, lr_d=P.LR_D, seed=2018):
    from neurec_amd.cfgan import CFGANEngine
    return CFGANEngine(tables, R_users_items, hg, hd, lr_g, lr_d, reg_g, reg_d, zr_ratio, zp_ratio, P.ZR_COEF, batch,
                       batch, opt_G=opt_g, opt_D=opt_d, mode=mode, seed=seed)


def _loss3(eng):
    import torch
    return torch.zeros(3, device=eng.dev)


def _clean(eng):
    for name, G in eng.G.items():
        assert not G.any().item(), name


def _golden_engine(g, case):
    mode, hg, hd, reg_g, reg_d, opt_g, opt_d = P.CASES[case][:7]
    M = sp.csr_matrix((np.ones(len(g["indices"]), np.float32), g["indices"], g["indptr"]), shape=tuple(g["shape"]))
    n_cols = M.shape[0] if mode == "itemBased" else M.shape[1]
    init = P.init_tables(n_cols, hg, hd, int(g["%s_init_seed" % case]))
    return _engine(init, M, hg, hd, mode, reg_g, reg_d, opt_g, opt_d, batch=max(P.BATCH_G, P.BATCH_D)), init


# ------------------------------------------------------------------ the reference's trace
@pytest.mark.parametrize("case", sorted(P.CASES))
def test_steps_match_the_reference_trace(golden, case):
    """The recorded run replayed through masks_given: every variable after every step of the first outer epoch and after
    the last step of the second against the float64 trace, under the trace's own f32-to-f64 distance; the three loss
    terms of every step against the float64 restatement; a d step leaves G's tables bit-unchanged and the reverse; each
    optimiser counts its own steps; the gradient buffers are zero again after every step."""
    g = golden
    eng, init = _golden_engine(g, case)
    r64, _ = restated(g, case)
    r32, _ = restated(g, case, np.float32)
    kinds = str(g["%s_kinds" % case])
    S1, names = len(kinds) // 2, list(init)
    loss = _loss3(eng)
    before = eng.tables()
    n_d = n_g = 0
    for s, kind in enumerate(kinds):
        B = int(g["%s_sizes" % case][s])
        rows = g["%s_rows" % case][s, :B]
        zr_b, pm_b = g["%s_zr" % case][s, :B], g["%s_pm" % case][s, :B]
        masks = eng.masks_given(rows, zr_b, pm_b)
        zr, pm = P.from_bits(zr_b, eng.n_cols), P.from_bits(pm_b, eng.n_cols)
        loss.zero_()
        if kind == "d":
            eng.d_step(rows, loss, masks)
            w64, w32 = r64.d_step(rows, zr, pm), r32.d_step(rows, zr, pm)
        else:
            eng.g_step(rows, loss, masks)
            w64, w32 = r64.g_step(rows, zr, pm), r32.g_step(rows, zr, pm)
        n_d, n_g = n_d + (kind == "d"), n_g + (kind == "g")
        assert (eng.dis.adam.t, eng.gen.adam.t) == (n_d, n_g)
        w64, w32 = np.asarray(w64, np.float64), np.asarray(w32, np.float64)
        _close(loss.cpu().numpy(), w64, np.abs(w32 - w64).max(), "%s step %d (%s) loss terms" % (case, s, kind))
        now = eng.tables()
        for k in names:
            if k.startswith("gen" if kind == "d" else "dis"):
                assert np.array_equal(now[k], before[k]), (case, s, kind, k)
            elif s < S1:
                _close(now[k], init[k].astype(np.float64) + g["%s_f64_%s" % (case, k)][s],
                       float(g["%s_gap_%s" % (case, k)][s]), "%s step %d %s" % (case, s, k))
        before = now
        _clean(eng)
    for k in names:
        _close(before[k], init[k].astype(np.float64) + g["%s_end_%s" % (case, k)], float(g["%s_endgap_%s" % (case, k)]),
               "%s end %s" % (case, k))


@pytest.mark.parametrize("case", ["user", "item"])
def test_the_ratings_match_the_reference(golden, case):
    """score() for every user and forward() on candidates after the recorded run, in both modes, under the distance of
    the reference's own float32 ratings from its float64 ones"""
    g = golden
    eng, init = _golden_engine(g, case)
    loss = _loss3(eng)
    for s, kind in enumerate(str(g["%s_kinds" % case])):
        B = int(g["%s_sizes" % case][s])
        rows = g["%s_rows" % case][s, :B]
        masks = eng.masks_given(rows, g["%s_zr" % case][s, :B], g["%s_pm" % case][s, :B])
        (eng.d_step if kind == "d" else eng.g_step)(rows, loss, masks)
    w64, w32 = g["%s_ratings_f64" % case], g["%s_ratings_f32" % case].astype(np.float64)
    bar = np.abs(w32 - w64).max()
    users = np.arange(27)
    got = eng.score(users).cpu().numpy()
    assert got.shape == (27, 131)
    _close(got, w64, bar, "%s ratings" % case)
    some = np.asarray([26, 0, 5, 5, 11])
    _close(eng.score(some).cpu().numpy(), w64[some], bar, "%s ratings of some users" % case)
    rs = np.random.RandomState(5)
    sizes = np.asarray([3, 0, 1, 7, 2])
    items = rs.randint(0, 131, int(sizes.sum()))
    want = np.concatenate([w64[u][items[a:a + n]] for u, a, n in zip(some, np.cumsum(sizes) - sizes, sizes)])
    _close(eng.forward(some, items, sizes).cpu().numpy(), want, bar, "%s candidates" % case)
    assert eng.score(np.zeros(0, np.int32)).shape == (0, 131) and eng.forward([], [], []).numel() == 0


# ------------------------------------------------------------------ the mask builder
def _rows_of_degree(n_rows, n_cols, deg, seed):
    rs = np.random.RandomState(seed)
    dense = np.zeros((n_rows, n_cols), np.float32)
    for r in range(n_rows):
        dense[r, rs.choice(n_cols, deg, replace=False)] = 1
    return sp.csr_matrix(dense)


@pytest.mark.parametrize("n_cols", [1, 31, 32, 33, 63, 64, 65, 131, 4099])
def test_the_mask_builder_is_its_restatement_bit_for_bit(n_cols):
    """degrees 0, 1, n_cols - 1 and n_cols, ratios 0, 0.3, 0.7 and 1, batches of 1, 2 and 65 rows (a row twice among
    them): both planes equal the restatement's words; the sample sizes are handed in, so a row without a train entry is
    sampled here as well"""
    for deg in sorted({0, 1, n_cols - 1, n_cols} - {-1}):
        if deg > n_cols:
            continue
        M = _rows_of_degree(65, n_cols, deg, seed=n_cols + deg)
        tables = P.init_tables(n_cols, [1], [1], 3)
        eng = _engine(tables, M, [1], [1], batch=65, seed=99)
        indptr, indices = M.indptr, M.indices
        for ratio in (0.0, 0.3, 0.7, 1.0):
            n = int((n_cols - deg) * ratio)
            for rows in (np.asarray([7]), np.asarray([3, 3]), np.arange(65)[::-1].copy()):
                counts = np.asarray([[n, int((n_cols - deg) * (1.0 - ratio))]] * len(rows))
                got_zr, got_pm = eng.masks_counts(rows, counts, epoch=6).host()
                want_zr, want_pm = P.masks(indptr, indices, rows, counts, n_cols, seed=99, epoch=6)
                assert np.array_equal(got_zr, want_zr) and np.array_equal(got_pm, want_pm), (n_cols, deg, ratio, len(rows))
        # the engine's own sizes: int((n_cols - deg) ratio), none for a row without a train entry
        zr, pm = eng.masks(np.arange(5), epoch=1).dense()
        for plane, ratio in ((zr, P.ZR_RATIO), (pm, P.ZP_RATIO)):
            assert (plane.sum(1) == deg + P.n_sample(n_cols, deg, ratio)).all()
            assert all(plane[r, indices[indptr[r]:indptr[r + 1]]].all() for r in range(5))


# ------------------------------------------------------------------ the steps on the edge shapes
def _random_train(n_rows, n_cols, seed, density=0.08):
    rs = np.random.RandomState(seed)
    dense = (rs.random_sample((n_rows, n_cols)) < density).astype(np.float32)
    return dense


EDGES = {
    # name: (hiddenLayer_G, hiddenLayer_D, batch rows, n_cols, opt_G, opt_D)
    "one_one": ([1], [1], [4], 33, "adam", "adam"),
    "odd_widths": ([3], [17], [0, 9], 131, "adam", "adam"),
    "wide_batch": ([16], [3], list(range(33)), 131, "adam", "adam"),
    "prime_cols": ([17], [16], list(range(33)), 4099, "adam", "adam"),
    "widest": ([125], [125], [2, 30], 4099, "adam", "adam"),
    "three_layers": ([16, 17, 3], [5, 3, 16], list(range(33)), 131, "adam", "adam"),
    "three_layers_sgd": ([16, 1, 125], [3, 17], list(range(1, 34)), 33, "sgd", "sgd"),
    "empty_rows": ([16], [17], [5, 6], 33, "adam", "sgd"),
    "one_column": ([3], [16], list(range(10, 43)), 131, "sgd", "adam"),
    "repeated_rows": ([17], [3], [8, 8, 2, 8, 2], 131, "adam", "adam"),
}


def _edge(name):
    hg, hd, rows, n_cols, opt_g, opt_d = EDGES[name]
    dense = _random_train(48, n_cols, seed=len(name) + n_cols)
    dense[[5, 6]] = 0                                           # two rows without a train entry
    if name == "one_column":
        dense[:, 7] = 1                                         # every row holds column 7
    tables = P.init_tables(n_cols, hg, hd, 17)
    rs = np.random.RandomState(23)
    for k in tables:
        if k.endswith("bias"):
            tables[k] = rs.uniform(-0.1, 0.1, tables[k].shape).astype(np.float32)
    return sp.csr_matrix(dense), tables, np.asarray(rows, np.int32)


def _run_edge(name):
    """(engine, per step: kind, tables, loss terms, masks) of d, g, d, g on the edge shape with the device's masks"""
    hg, hd, _, n_cols, opt_g, opt_d = EDGES[name]
    M, tables, rows = _edge(name)
    eng = _engine(tables, M, hg, hd, reg_g=0.01, reg_d=0.02, opt_g=opt_g, opt_d=opt_d, batch=len(rows), lr_g=0.01,
                  lr_d=0.01)
    loss, out = _loss3(eng), []
    for s, kind in enumerate("dgdg"):
        eng.epoch = s // 2
        masks = eng.masks(rows)
        loss.zero_()
        (eng.d_step if kind == "d" else eng.g_step)(rows, loss, masks)
        _clean(eng)
        out.append((kind, eng.tables(), loss.cpu().numpy().copy(), masks.dense()))
    return eng, out


@pytest.mark.parametrize("name", sorted(EDGES))
def test_steps_on_the_edge_shapes_match_the_restatement(name):
    """d, g, d, g with the device's own masks against the float64 restatement fed the same masks: every variable and
    the loss terms after every step within 4 x the float32 restatement's distance plus 1e-5 max|want|; the untouched
    network bit-unchanged; a second run of the same steps is bit-identical"""
    hg, hd, _, n_cols, opt_g, opt_d = EDGES[name]
    M, tables, rows = _edge(name)
    eng, steps = _run_edge(name)
    mk = lambda dt: P.CFGAN(tables, M, 0.01, 0.01, 0.01, 0.02, P.ZR_COEF, opt_g, opt_d, dt)     # noqa: E731
    r64, r32 = mk(np.float64), mk(np.float32)
    before = {k: np.asarray(v, np.float32) for k, v in tables.items()}
    for s, (kind, now, loss, (zr, pm)) in enumerate(steps):
        pos = np.asarray(M[rows].todense()) > 0
        assert (zr >= pos).all() and (pm >= pos).all() and not zr[~pos.any(1)].any() and not pm[~pos.any(1)].any()
        fn = "d_step" if kind == "d" else "g_step"
        w64, w32 = (np.asarray(getattr(r, fn)(rows, zr, pm), np.float64) for r in (r64, r32))
        _close(loss, w64, np.abs(w32 - w64).max(), "%s step %d (%s) loss terms" % (name, s, kind))
        for k in now:
            if k.startswith("gen" if kind == "d" else "dis"):
                assert np.array_equal(now[k], before[k]), (name, s, k)
            else:
                _close(now[k], r64.T[k], np.abs(r32.T[k].astype(np.float64) - r64.T[k]).max(),
                       "%s step %d %s" % (name, s, k))
        before = now
    _, again = _run_edge(name)
    for (_, a, la, _), (_, b, lb, _) in zip(steps, again):
        assert np.array_equal(la, lb) and all(np.array_equal(a[k], b[k]) for k in a), name


def test_refusals_and_empty_work():
    import torch
    M, tables, rows = _edge("odd_widths")
    eng = _engine(tables, M, [3], [17], batch=4)
    loss, before = _loss3(eng), eng.tables()
    eng.d_step(np.zeros(0, np.int32), loss)
    eng.g_step([], loss)
    assert (eng.dis.adam.t, eng.gen.adam.t) == (0, 0) and not loss.any().item()
    assert all(np.array_equal(v, before[k]) for k, v in eng.tables().items())
    assert eng.masks([]).zr.shape == (0, eng.words)
    with pytest.raises(ValueError, match="a batch of 5 rows, the engine was made for 4"):
        eng.d_step(np.arange(5), loss)
    with pytest.raises(ValueError, match=r"row ids must lie in \[0, 48\)"):
        eng.g_step([48], loss)
    with pytest.raises(ValueError, match="the masks were made for other rows"):
        eng.d_step([1, 2], loss, eng.masks([2, 1]))
    with pytest.raises(ValueError, match="a mask row holds 4 words, 5 expected"):
        eng.masks_given([1], np.zeros((1, 4), np.uint32), np.zeros((1, 4), np.uint32))
    with pytest.raises(ValueError, match="mask bits beyond column 131"):
        eng.masks_given([1], np.full((1, 5), 0xffffffff, np.uint32), np.zeros((1, 5), np.uint32))
    with pytest.raises(NotImplementedError, match=r"hiddenLayer_G=\[513\]"):
        _engine(tables, M, [513], [17])
    with pytest.raises(NotImplementedError, match="batchSize_G=1025"):
        _engine(tables, M, [3], [17], batch=1025)
    with pytest.raises(ValueError, match=r"gen_h0_kernel must be \[131, 4\]"):
        _engine(tables, M, [4], [17])
    with pytest.raises(ValueError, match="user ids must lie in"):
        eng.score([48])
    assert torch.isfinite(eng.score([0, 5]).cpu()).all()


def test_cfgan_config_drops_in(tmp_path):
    """NeuRec.properties + conf/CFGAN.properties on ml-100k through neurec_amd.main in a fresh child process, two outer
    epochs in each mode at small widths: the reference's log lines, finite loss terms, the step counts of the schedule"""
    code = r"""
import json, os, re, sys
import numpy as np
sys.path.insert(0, %r)
from test_gru4rec_gpu import _run
out = {}
for mode in ("userBased", "itemBased"):
    tmp = os.path.join(%r, mode)
    model = _run(tmp, ["--recommender=CFGAN", "--epochs=2", "--mode=" + mode, "--hiddenLayer_G=[32]", "--hiddenLayer_D=[16]",
                       "--batchSize_G=64", "--batchSize_D=128"])
    folder = os.path.join(tmp, "log", "ml-100k", "CFGAN")
    files = os.listdir(folder)
    text = open(os.path.join(folder, files[0])).read()
    eng = model.engine
    out[mode] = dict(files=len(files), epochs=[int(n) for n in re.findall(r"epoch (\d+):\t", text)],
                     header="metrics:\t" in text, params="CFGAN's hyperparameters:" in text,
                     t=[eng.dis.adam.t, eng.gen.adam.t], rows=eng.n_rows, cols=eng.n_cols,
                     finite=bool(np.isfinite(model.losses_d.cpu().numpy()).all() and
                                 np.isfinite(model.losses_g.cpu().numpy()).all()),
                     positive=bool(model.losses_d.cpu().numpy()[:, :2].min() > 0),
                     scores=list(model.predict([0, 1], None).shape))
print("RESULT " + json.dumps(out))
""" % (os.path.dirname(os.path.abspath(__file__)), str(tmp_path))
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    out = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for mode, res in out.items():
        assert res["files"] == 1 and res["epochs"] == [0, 1] and res["header"] and res["params"], (mode, res)
        assert res["t"] == [2 * -(-res["rows"] // 128), 2 * -(-res["rows"] // 64)] and res["finite"] and res["positive"]
        assert res["scores"][0] == 2
    assert out["userBased"]["cols"] == out["itemBased"]["rows"] == out["userBased"]["scores"][1]
