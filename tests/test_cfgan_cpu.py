"""CFGAN without a GPU: the numpy restatement against torch autograd and against the reference's trace after every step,
the mask builder's restatement, the plugin's schedule and log lines, the defaults and the refusals."""
import configparser
import inspect
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import cfgan_restatement as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "tfgraph_cfgan.npz"))


def train_of(g, case):
    """the model's R for a case: the train matrix, transposed for itemBased"""
    M = sp.csr_matrix((np.ones(len(g["indices"]), np.float32), g["indices"], g["indptr"]), shape=tuple(g["shape"]))
    return (M.T if P.CASES[case][0] == "itemBased" else M).tocsr()


def restated(g, case, dtype=np.float64):
    mode, hg, hd, reg_g, reg_d, opt_g, opt_d = P.CASES[case][:7]
    R = train_of(g, case)
    init = P.init_tables(R.shape[1], hg, hd, int(g["%s_init_seed" % case]))
    return P.CFGAN(init, R, P.LR_G, P.LR_D, reg_g, reg_d, P.ZR_COEF, opt_g, opt_d, dtype), init


def replay(g, case, model, upto=None):
    """the recorded steps on a restatement; yields (step, kind) after each"""
    kinds, n_cols = str(g["%s_kinds" % case]), model.n_cols
    for s, kind in enumerate(kinds[:upto]):
        B = int(g["%s_sizes" % case][s])
        rows = g["%s_rows" % case][s, :B]
        zr, pm = (P.from_bits(g["%s_%s" % (case, p)][s, :B], n_cols) for p in ("zr", "pm"))
        (model.d_step if kind == "d" else model.g_step)(rows, zr, pm)
        yield s, kind


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", ["user", "deep"])
def test_the_restated_gradients_are_autograd_s(case):
    """both losses written out in torch (float64, CPU) and differentiated by autograd: the restatement's hand-written
    gradients of every variable of the stepped network, and its loss terms (no fixture: a matrix and tables of its own)"""
    import torch
    mode, hg, hd, reg_g, reg_d, opt_g, opt_d = P.CASES[case][:7]
    rs0 = np.random.RandomState(8)
    dense = (rs0.random_sample((14, 37)) < 0.15).astype(np.float32)
    dense[5], dense[11] = 0, rs0.random_sample(37) < 0.7
    tables = P.init_tables(37, hg, hd, 41)
    for k in tables:
        if k.endswith("bias"):
            tables[k] = rs0.uniform(-0.2, 0.2, tables[k].shape).astype(np.float32)
    model = P.CFGAN(tables, sp.csr_matrix(dense), P.LR_G, P.LR_D, reg_g, 0.02, P.ZR_COEF, opt_g, opt_d)
    n, rs = model.n_cols, np.random.RandomState(3)
    rows = np.asarray([0, 5, 11, 11, 2])                       # an empty row, a long row twice
    zr, pm = rs.random_sample((5, n)) < 0.6, rs.random_sample((5, n)) < 0.5
    T = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in model.T.items()}
    c = torch.tensor(model.rows(rows))

    def net(x, name):
        layers = P.layers_of(T, name)
        for k, (W, b) in enumerate(layers):
            x = x @ W + b
            x = x if k == len(layers) - 1 else torch.sigmoid(x)
        return x
    sp_ = torch.nn.functional.softplus
    out = net(c, "gen")
    fake = net(torch.cat([c, out * torch.tensor(pm, dtype=torch.float64)], 1), "dis")
    real = net(torch.cat([c, c], 1), "dis")
    l2 = lambda name: sum((v * v).sum() for k, v in T.items() if k.startswith(name)) / 2     # noqa: E731
    d_loss = sp_(-real).mean() + sp_(fake).mean() + float(model.reg_D) * l2("dis")
    g_loss = sp_(-fake).mean() + float(model.reg_G) * l2("gen") + \
        float(model.zr_coef) * (out * out * torch.tensor(zr, dtype=torch.float64)).sum(1).mean()
    for loss, fn, name in ((d_loss, model.d_gradients, "dis"), (g_loss, model.g_gradients, "gen")):
        terms, grads = fn(rows, zr, pm)
        assert abs(float(loss.detach()) - float(sum(terms))) <= 1e-12 * abs(float(loss.detach()))
        keys = [k for k in T if k.startswith(name)]
        assert sorted(grads) == sorted(keys)
        for k, want in zip(keys, torch.autograd.grad(loss, [T[k] for k in keys], retain_graph=True)):
            err = np.abs(grads[k] - want.numpy()).max()
            assert err <= 1e-12 * max(np.abs(want.numpy()).max(), 1e-3), (case, k, err)


@pytest.mark.parametrize("case", sorted(P.CASES))
def test_the_restatement_follows_the_reference_trace(golden, case):
    """every variable after every recorded step of the first outer epoch, and after the last step of the second, against
    the reference's float64 run; a d step leaves every gen_* table bit-unchanged and the reverse; each optimiser's step
    count advances on its own steps only"""
    g = golden
    model, init = restated(g, case)
    kinds = str(g["%s_kinds" % case])
    S1 = len(kinds) // 2
    names = P.names(len(P.CASES[case][1]), len(P.CASES[case][2]))
    assert list(model.T) == names
    n_d = n_g = 0
    before = {k: v.copy() for k, v in model.T.items()}
    for s, kind in replay(g, case, model):
        n_d, n_g = n_d + (kind == "d"), n_g + (kind == "g")
        assert (model.opt_D.t, model.opt_G.t) == (n_d, n_g)
        for k in names:
            moved = not np.array_equal(before[k], model.T[k])
            assert moved == k.startswith("dis" if kind == "d" else "gen"), (case, s, kind, k)
            if s < S1:
                want = init[k].astype(np.float64) + g["%s_f64_%s" % (case, k)][s]
                assert np.abs(model.T[k] - want).max() <= 1e-11, (case, s, k)
        before = {k: v.copy() for k, v in model.T.items()}
    for k in names:
        want = init[k].astype(np.float64) + g["%s_end_%s" % (case, k)]
        assert np.abs(model.T[k] - want).max() <= 1e-10, (case, k)
    if "%s_ratings_f64" % case in g.files:
        got = model.ratings()
        got = got.T if P.CASES[case][0] == "itemBased" else got
        assert got.shape == tuple(g["shape"]) and np.abs(got - g["%s_ratings_f64" % case]).max() <= 1e-10


def test_the_trace_holds_what_the_issue_names(golden):
    g = golden
    assert tuple(g["shape"]) == (27, 131) and g["indptr"][6] == g["indptr"][5]          # user 5 has no train item
    M = train_of(g, "user")
    assert sorted(g["cases"].tolist()) == sorted(P.CASES)
    for case in ("user", "deep", "steps"):
        rows, sizes = g["%s_rows" % case], g["%s_sizes" % case]
        assert any(5 in r[:n] for r, n in zip(rows, sizes))
        assert any(M[r[:n]][:, 3].nnz > 1 for r, n in zip(rows, sizes))
        s = next(s for s, (r, n) in enumerate(zip(rows, sizes)) if 5 in r[:n])
        b = list(rows[s]).index(5)
        assert not g["%s_pm" % case][s, b].any() and not g["%s_zr" % case][s, b].any()      # empty masks, in the batch
    assert str(g["steps_kinds"]) == "ddddgggg" * 2 and str(g["user_kinds"]) == "ddgg" * 2
    # the masks hold the positives plus exactly int((n - deg) ratio) others
    case = "user"
    kinds = str(g["user_kinds"])
    for s, kind in enumerate(kinds):
        n = int(g["user_sizes"][s])
        for b, r in enumerate(g["user_rows"][s, :n]):
            pos = M[r].indices
            for plane, ratio in (("zr", P.ZR_RATIO), ("pm", P.ZP_RATIO)):
                if plane == "zr" and kind == "d":
                    continue
                bits = P.from_bits(g["user_%s" % plane][s, b], 131)[0]
                assert bits[pos].all() and bits.sum() == len(pos) + P.n_sample(131, len(pos), ratio)


# ------------------------------------------------------------------ the mask builder
def _toy(n_rows, n_cols, deg, seed=0):
    rs = np.random.RandomState(seed)
    rows = [np.sort(rs.choice(n_cols, deg, replace=False)) for _ in range(n_rows)]
    indptr = np.arange(n_rows + 1, dtype=np.int64) * deg
    return indptr, (np.concatenate(rows) if deg else np.zeros(0, np.int64)).astype(np.int32)


def test_the_masks_have_exact_sizes_and_depend_on_their_key_alone():
    n_cols, deg = 131, 9
    indptr, indices = _toy(6, n_cols, deg)
    rows = np.arange(6)
    for ratio in (0.0, 0.3, 0.7, 1.0):
        n = P.n_sample(n_cols, deg, ratio)
        counts = np.full((6, 2), n)
        zr, pm = P.masks(indptr, indices, rows, counts, n_cols, seed=2018, epoch=4)
        for plane in (zr, pm):
            dense = P.from_bits(plane, n_cols)
            assert (dense.sum(1) == deg + int((n_cols - deg) * ratio)).all()
            assert all(dense[r, indices[indptr[r]:indptr[r + 1]]].all() for r in rows)
            assert not (plane[:, -1] >> np.uint32(n_cols % 32)).any()              # no bit beyond the last column
        if 0 < n < n_cols - deg:
            assert not np.array_equal(zr, pm)                                      # the planes are drawn independently
            zr2, _ = P.masks(indptr, indices, rows, counts, n_cols, seed=2018, epoch=5)
            assert not np.array_equal(zr, zr2)                                     # another epoch, other masks
            zr3, _ = P.masks(indptr, indices, rows, counts, n_cols, seed=2019, epoch=4)
            assert not np.array_equal(zr, zr3)
        # the same key gives the same bits: alone, in another batch order, twice in a batch
        again, _ = P.masks(indptr, indices, rows[::-1], counts, n_cols, seed=2018, epoch=4)
        assert np.array_equal(again[::-1], zr)
        twice, _ = P.masks(indptr, indices, np.asarray([2, 2]), counts[:2], n_cols, seed=2018, epoch=4)
        assert np.array_equal(twice[0], zr[2]) and np.array_equal(twice[1], zr[2])
    assert P.n_sample(n_cols, 0, 0.7) == 0 and P.n_sample(n_cols, n_cols, 0.7) == 0
    assert P.n_sample(41, 3, 0.7) == int(38 * 0.7) == 26


def test_the_mask_ties_fall_to_the_lower_column(monkeypatch):
    """two columns with one key: the pair (key, column) decides"""
    monkeypatch.setattr(P, "column_keys", lambda *a: np.asarray([5, 1, 5, 5, 0, 9], np.int64))
    got = P.mask_row([4], 6, 3, 0, 0, 0, 0)
    assert got.tolist() == [True, True, True, False, True, False]


def test_the_sample_is_uniform_over_the_free_columns():
    """4,096 rows of one degree, n_cols = 97, ratio 0.5: every free column's inclusion count within 6 standard
    deviations of its binomial mean"""
    n_rows, n_cols, deg = 4096, 97, 7
    indptr, indices = _toy(n_rows, n_cols, deg, seed=11)
    n = P.n_sample(n_cols, deg, 0.5)
    assert n == 45
    hits, free = np.zeros(n_cols), np.zeros(n_cols)
    for r in range(n_rows):
        pos = indices[indptr[r]:indptr[r + 1]]
        m = P.mask_row(pos, n_cols, n, 2018, 0, 1, r)
        m[pos] = False
        hits += m
        free += 1
        free[pos] -= 1
    p = n / float(n_cols - deg)
    z = (hits - free * p) / np.sqrt(free * p * (1 - p))
    assert np.abs(z).max() < 6.0, np.abs(z).max()


# ------------------------------------------------------------------ the plugin on the host
def test_find_recommender_resolves_cfgan():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import AbstractRecommender
    cls = find_recommender("CFGAN")
    assert cls.__module__ == "neurec_amd.model.general_recommender.CFGAN" and issubclass(cls, AbstractRecommender)
    doc = sys.modules[cls.__module__].__doc__
    assert "As the reference" in doc and "Deviations" in doc
    keys = re.findall(r'conf\["(\w+)"\]', inspect.getsource(cls.__init__))
    assert keys == ["epochs", "mode", "reg_G", "reg_D", "lr_G", "lr_D", "batchSize_G", "batchSize_D", "opt_G", "opt_D",
                    "hiddenLayer_G", "hiddenLayer_D", "step_G", "step_D", "ZR_ratio", "ZP_ratio", "ZR_coefficient",
                    "verbose"]


def test_the_defaults_row_equals_the_properties_file(tmp_path):
    from neurec_amd import defaults
    ref = configparser.ConfigParser()
    ref.optionxform = str
    assert ref.read(os.path.join(GOLDEN, "neurec_conf", "conf", "CFGAN.properties"))
    want = dict(ref["hyperparameters"])
    assert dict(defaults.MODELS["CFGAN"]) == want and [k for k, _ in defaults.MODELS["CFGAN"]] == list(want)
    path = defaults.write_default_configs(str(tmp_path))
    from neurec_amd.util.configurator import Configurator
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=CFGAN"])
    finally:
        os.chdir(cwd)
    assert (conf["hiddenLayer_G"], conf["hiddenLayer_D"], conf["batchSize_G"], conf["batchSize_D"]) == ([400], [125], 32, 64)
    assert (conf["mode"], conf["opt_G"], conf["ZR_ratio"], conf["ZR_coefficient"]) == ("userBased", "adam", 0.7, 0.03)


class _Engine:
    dev = "cpu"

    def __init__(self):
        self.calls, self.epoch = [], None

    def d_step(self, rows, loss_out, masks=None):
        self.calls.append(("d", self.epoch, np.asarray(rows).copy()))

    def g_step(self, rows, loss_out, masks=None):
        self.calls.append(("g", self.epoch, np.asarray(rows).copy()))


@pytest.mark.parametrize("case", ["user", "item", "steps"])
def test_the_plugin_runs_the_recorded_schedule_and_logs_its_lines(golden, case):
    """train_model() on a recording engine against the reference's recorded run: the same sequence of trainer runs with
    the same batch sizes, every pass a permutation of all rows, the masks' epoch per outer epoch, the same log lines"""
    from neurec_amd.model.general_recommender.CFGAN import CFGAN
    g = golden
    mode, hg, hd, reg_g, reg_d, opt_g, opt_d, step_d, step_g = P.CASES[case]
    lines = []
    model = CFGAN.__new__(CFGAN)
    model.logger = type("L", (), {"info": staticmethod(lambda m: lines.append(str(m)))})()
    model.evaluator = type("E", (), {"metrics_info": staticmethod(lambda: "metrics"),
                                     "evaluate": staticmethod(lambda m: "recorded")})()
    model.engine = _Engine()
    R = train_of(g, case)
    model.num_rows, model.num_cols = R.shape
    model.batchSize_G, model.batchSize_D, model.step_G, model.step_D = P.BATCH_G, P.BATCH_D, step_g, step_d
    model.epochs, model.verbose = 2 * step_g, 1
    model.train_model()
    calls = model.engine.calls
    assert "".join(k for k, _, _ in calls) == str(g["%s_kinds" % case])
    assert [len(r) for _, _, r in calls] == g["%s_sizes" % case].tolist()
    half = len(calls) // 2
    assert [e for _, e, _ in calls] == [0] * half + [1] * half
    at = 0
    for kind, per in (("d", -(-R.shape[0] // P.BATCH_D)), ("g", -(-R.shape[0] // P.BATCH_G))):
        for _ in range(step_d if kind == "d" else step_g):
            seen = np.concatenate([r for _, _, r in calls[at:at + per]])
            assert sorted(seen.tolist()) == list(range(R.shape[0]))
            at += per
    assert lines == g["%s_log" % case].tolist()[2:] == ["metrics", "epoch 0:\trecorded", "epoch 1:\trecorded"]
    model.epochs, model.verbose, lines[:] = 3 * step_g, 2, []
    model.train_model()
    assert lines == ["metrics", "epoch 0:\trecorded", "epoch 2:\trecorded"]
    model.epochs, model.step_G, model.engine.calls = 5, 2, []           # int(5 / 2) = 2 outer epochs
    model.train_model()
    assert max(e for _, e, _ in model.engine.calls) == 1


def test_the_refusals_name_the_key_and_the_range(monkeypatch):
    from neurec_amd.cfgan import check_config
    ok = dict(mode="userBased", hidden_g=[400], hidden_d=[125], batch_g=32, batch_d=64, opt_g="adam", opt_d="sgd",
              zr_ratio=0.7, zp_ratio=0.0)
    check_config(**ok)
    check_config(**dict(ok, mode="itemBased", hidden_g=[1, 512, 3], zr_ratio=1.0, batch_d=1024))
    for change, exc, text in ((dict(mode="both"), ValueError, r"mode='both' is not supported \(userBased or itemBased\)"),
                              (dict(opt_g="adagrad"), ValueError, r"opt_G='adagrad' is not supported \(adam or sgd\)"),
                              (dict(opt_d="rmsprop"), ValueError, r"opt_D='rmsprop' is not supported"),
                              (dict(hidden_g=[]), NotImplementedError, r"hiddenLayer_G=\[\] is not supported \(1 to 3"),
                              (dict(hidden_d=[8, 8, 8, 8]), NotImplementedError, r"hiddenLayer_D=.* \(1 to 3 hidden"),
                              (dict(hidden_g=[513]), NotImplementedError, r"hiddenLayer_G=\[513\] .*widths 1 to 512"),
                              (dict(hidden_d=[0]), NotImplementedError, r"hiddenLayer_D=\[0\]"),
                              (dict(batch_g=1025), NotImplementedError, r"batchSize_G=1025 is not supported \(1 to 1024"),
                              (dict(batch_d=0), NotImplementedError, r"batchSize_D=0"),
                              (dict(zr_ratio=1.5), ValueError, r"ZR_ratio=1.5 is not supported \(0 to 1\)"),
                              (dict(zp_ratio=-0.1), ValueError, r"ZP_ratio=-0.1")):
        with pytest.raises(exc, match=text):
            check_config(**dict(ok, **change))
    from neurec_amd.model.general_recommender.CFGAN import CFGAN
    from neurec_amd import parallel
    model = CFGAN.__new__(CFGAN)
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)
    with pytest.raises(NotImplementedError, match="CFGAN runs on one GPU"):
        model.build_graph()


def test_the_c_entries_refuse_by_name():
    import ctypes as C
    from neurec_amd import _lib
    a = _lib.CfganStepArgs()
    floats, nbytes = C.c_size_t(0), C.c_size_t(0)
    a.gen.n_hidden, a.dis.n_hidden, a.n_cols, a.max_batch = 4, 1, 131, 8
    with pytest.raises(NotImplementedError, match=r"4 hidden layers are not supported \(1 to 3\)"):
        _lib.call("nrhip_cfgan_workspace", C.byref(a), C.byref(floats), C.byref(nbytes))
    a.gen.n_hidden = 1
    a.gen.width[0], a.dis.width[0] = 513, 10
    with pytest.raises(NotImplementedError, match=r"a hidden layer of 513 units is not supported \(1 to 512\)"):
        _lib.call("nrhip_cfgan_workspace", C.byref(a), C.byref(floats), C.byref(nbytes))
    a.gen.width[0], a.max_batch = 24, 1025
    with pytest.raises(NotImplementedError, match=r"a batch of 1025 rows is not supported \(up to 1024\)"):
        _lib.call("nrhip_cfgan_workspace", C.byref(a), C.byref(floats), C.byref(nbytes))
    a.max_batch = 16
    _lib.call("nrhip_cfgan_workspace", C.byref(a), C.byref(floats), C.byref(nbytes))
    assert floats.value >= 2 * 16 * 131 + 16 * 24 * 2 + 32 * 10 * 2 and nbytes.value == 0     # n_cols <= 1024: no split
    a.n_cols = 41000
    big = C.c_size_t(0)
    _lib.call("nrhip_cfgan_workspace", C.byref(a), C.byref(big), C.byref(nbytes))
    assert big.value > floats.value and nbytes.value > 0
    with pytest.raises(ValueError, match="null argument"):
        _lib.call("nrhip_cfgan_d_step", None, None)
    _lib.call("nrhip_cfgan_masks", None, None, None, None, 0, 0, 131, 1, 0, None, None, None)     # an empty batch
    with pytest.raises(ValueError, match="cfgan_masks: null argument"):
        _lib.call("nrhip_cfgan_masks", None, None, None, None, 2, 5, 131, 1, 0, None, None, None)
