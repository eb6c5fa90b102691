"""IRGAN without a GPU: the numpy restatement against torch autograd and against the reference's trace after every step,
both draw rules against their distributions, the plugin's constructor, schedule and log lines on a stub engine, the
refusals, the defaults and the pretrain_file branches."""
import configparser
import inspect
import os
import pickle
import re
import sys

import numpy as np
import pytest

import irgan_restatement as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "tfgraph_irgan.npz"))


def restated(g, case, dtype=np.float64):
    g_reg, d_reg = P.CASES[case][:2]
    U, I = (int(x) for x in g["shape"])
    init = P.init_tables(U, I, P.FACTORS, int(g["%s_init_seed" % case]))
    return P.IRGAN(init, g["indptr"], g["indices"], P.LR, g_reg, d_reg, dtype), init


def recorded_steps(g, case):
    """(kind, arguments) of every recorded step in the order run: ('d', (users, items, labels)), ('g', (user, samples))"""
    nd = ng = 0
    for kind in str(g["%s_kinds" % case]):
        if kind == "d":
            B = int(g["%s_d_sizes" % case][nd])
            yield kind, tuple(g["%s_d_%s" % (case, k)][nd, :B] for k in ("users", "items", "labels"))
            nd += 1
        else:
            S = int(g["%s_g_sizes" % case][ng])
            yield kind, (int(g["%s_g_user" % case][ng]), g["%s_g_samples" % case][ng, :S])
            ng += 1


def wanted(g, case, init, name, n):
    """the float64 table `name` after the n-th step (from 0) of its network in the first epoch"""
    return init[name].astype(np.float64) + g["%s_f64_%s" % (case, name)][n]


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", sorted(P.CASES))
def test_the_restatement_follows_the_reference_trace(golden, case):
    """every table of the stepped network after every recorded step of the first epoch, and all six after the last step
    of the second, against the reference's float64 run to 1e-11; the other network is bit-unchanged by a step.  A
    regulariser counted once instead of B times, or a train-user rule other than any(), does not pass."""
    g = golden
    model, init = restated(g, case)
    kinds = str(g["%s_kinds" % case])
    S1 = len(kinds) // 2
    n = {"d": 0, "g": 0}
    for s, (kind, args) in enumerate(recorded_steps(g, case)):
        before = {k: v.copy() for k, v in model.T.items()}
        (model.d_step if kind == "d" else model.g_step)(*args)
        for k in P.NAMES:
            if k[0] != kind:
                assert np.array_equal(before[k], model.T[k]), (case, s, k)
            elif s < S1:
                assert np.abs(model.T[k] - wanted(g, case, init, k, n[kind])).max() <= 1e-11, (case, s, k)
        n[kind] += 1
    for k in P.NAMES:
        assert np.abs(model.T[k] - (init[k].astype(np.float64) + g["%s_end_%s" % (case, k)])).max() <= 1e-11, (case, k)
    assert np.abs(model.ratings() - g["%s_ratings_f64" % case]).max() <= 1e-11


def test_the_restated_gradients_are_autograd_s():
    """both stated losses written out in torch (float64, CPU): a D batch with one pair three times under different
    labels and several pairs of one user; a G step with repeated samples, positives among them, and g_reg > 0"""
    import torch
    rs = np.random.RandomState(5)
    U, I, d = 6, 11, 3
    dense = rs.random_sample((U, I)) < 0.4
    dense[2] = False
    dense[3, [0, 4, 7]] = True
    indptr = np.concatenate([[0], np.cumsum(dense.sum(1))])
    indices = np.nonzero(dense)[1]
    tables = P.init_tables(U, I, d, 9)
    tables["d_b"] = rs.uniform(-0.2, 0.2, I).astype(np.float32)
    model = P.IRGAN(tables, indptr, indices, 0.05, 0.03, 0.02)
    T = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in model.T.items()}
    users, items = np.asarray([3, 1, 3, 3, 0, 3]), np.asarray([4, 2, 4, 4, 2, 9])
    labels = np.asarray([1.0, 0.0, 0.0, 1.0, 1.0, 0.0])
    tu, ti, ty = torch.tensor(users), torch.tensor(items), torch.tensor(labels)
    x = (T["d_P"][tu] * T["d_Q"][ti]).sum(1) + T["d_b"][ti]
    ce = torch.clamp(x, min=0) - x * ty + torch.log1p(torch.exp(-x.abs()))
    l2 = ((T["d_P"][tu] ** 2).sum() + (T["d_Q"][ti] ** 2).sum() + (T["d_b"][ti] ** 2).sum()) / 2
    d_loss = (ce + 0.02 * l2).sum()                               # the vector pre_loss, summed: B times the regulariser
    terms, grads = model.d_gradients(users, items, labels)
    assert abs(float(d_loss.detach()) - float(sum(terms))) <= 1e-12 * abs(float(d_loss.detach()))
    for k, want in zip(("d_P", "d_Q", "d_b"), torch.autograd.grad(d_loss, [T["d_P"], T["d_Q"], T["d_b"]])):
        assert np.abs(grads[k] - want.numpy()).max() <= 1e-12 * max(np.abs(want.numpy()).max(), 1e-3), k
    user, samples = 3, np.asarray([4, 4, 9, 0, 4, 1])
    _, r = model.rewards(user, samples)
    ts = torch.tensor(samples)
    p = torch.softmax((T["g_Q"] * T["g_P"][user]).sum(1) + T["g_b"], 0)
    g_loss = -(torch.log(p[ts]) * torch.tensor(r)).mean() + \
        0.03 * ((T["g_P"][user] ** 2).sum() + (T["g_Q"][ts] ** 2).sum() + (T["g_b"][ts] ** 2).sum()) / 2
    grads = model.g_gradients(user, samples)
    for k, want in zip(("g_P", "g_Q", "g_b"), torch.autograd.grad(g_loss, [T["g_P"], T["g_Q"], T["g_b"]])):
        assert np.abs(grads[k] - want.numpy()).max() <= 1e-12 * max(np.abs(want.numpy()).max(), 1e-3), k


def test_the_trace_holds_what_the_issue_names(golden):
    g = golden
    assert tuple(g["shape"]) == (23, 67) and sorted(g["cases"].tolist()) == sorted(P.CASES)
    indptr, indices = g["indptr"], g["indices"]
    row = lambda u: indices[indptr[u]:indptr[u + 1]].tolist()       # noqa: E731
    assert row(4) == [] and row(9) == [0] and row(2)[0] == 0 and len(row(2)) > 1 and len(row(13)) == 1
    assert len(row(11)) >= 20
    train = P.train_users(indptr, indices)
    assert 4 not in train and 9 not in train and 2 in train and 13 in train and len(train) == 21
    nnz = sum(len(row(u)) for u in train)
    for case, (g_reg, d_reg, d_tau, d_epoch, g_epoch) in P.CASES.items():
        per_d = -(-2 * nnz // P.BATCH)
        assert str(g["%s_kinds" % case]) == ("d" * per_d * d_epoch + "g" * len(train) * g_epoch) * 2
        assert g["%s_g_user" % case].tolist() == train * (2 * g_epoch)           # ascending, the skipped users absent
        assert g["%s_g_sizes" % case].tolist() == [2 * len(row(u)) for u in train] * (2 * g_epoch)
        ptr = g["%s_pass_ptr" % case]
        assert len(ptr) == 2 * d_epoch + 1 and (np.diff(ptr) == 2 * nnz).all()
        users, items, labels = (g["%s_pass_%s" % (case, k)] for k in ("users", "items", "labels"))
        order, at = g["%s_pass_order" % case], 0
        for n in range(2 * d_epoch):
            u, i, y = (x[ptr[n]:ptr[n + 1]] for x in (users, items, labels))
            assert u[0::2].tolist() == u[1::2].tolist() == [w for w in train for _ in row(w)]
            assert i[0::2].tolist() == [j for w in train for j in row(w)]
            assert (y[0::2] == 1).all() and (y[1::2] == 0).all()
            o = order[ptr[n]:ptr[n + 1]]
            assert sorted(o.tolist()) == list(range(2 * nnz))
            for s in range(per_d):                                  # the fed batches are the pass's triples in that order
                B = int(g["%s_d_sizes" % case][at])
                idx = o[s * P.BATCH:s * P.BATCH + B]
                assert B == min(P.BATCH, 2 * nnz - s * P.BATCH)
                assert np.array_equal(g["%s_d_users" % case][at, :B], u[idx])
                assert np.array_equal(g["%s_d_items" % case][at, :B], i[idx])
                assert np.array_equal(g["%s_d_labels" % case][at, :B], y[idx])
                at += 1
        assert g["%s_log" % case].tolist()[2:] == ["recorded"] * (2 * g_epoch)
    # positives are not excluded from D's negatives: some recorded negative is a train item of its user
    assert any(int(i) in row(int(u)) for u, i, y in zip(g["steps_pass_users"], g["steps_pass_items"],
                                                        g["steps_pass_labels"]) if y == 0)


# ------------------------------------------------------------------ the draw rules
N_DRAWS = 200000
SEVEN = np.asarray([0.3, -0.1, 0.0, 0.25, -1e4, 0.1, -0.3])         # the fifth gets weight 0 at tau = 0.2


def _within(counts, prob, n):
    sd = np.sqrt(prob * (1 - prob) / n)
    z = np.abs(counts / n - prob) / np.where(sd > 0, sd, 1.0)
    assert (counts[prob == 0] == 0).all() and z.max() < 5.0, z


def test_the_plain_draw_rule_reproduces_its_distribution():
    w = P.weights(SEVEN, 0.2)
    assert w[4] == 0 and w.max() == 2 ** 31 and (w[[0, 1, 2, 3, 5, 6]] > 0).all()
    got = P.plain_draws(w, N_DRAWS, seed=2018, pas=3, user=11)
    _within(np.bincount(got, minlength=7).astype(np.float64), w / float(w.sum()), N_DRAWS)
    again = P.plain_draws(w, 50, seed=2018, pas=3, user=11)
    assert np.array_equal(again, got[:50])                          # a draw depends on its own key alone
    assert not np.array_equal(P.plain_draws(w, 50, seed=2018, pas=4, user=11), again)
    assert not np.array_equal(P.plain_draws(w, 50, seed=2018, pas=3, user=12), again)


def test_the_mixture_draw_rule_reproduces_pn():
    w = P.weights(SEVEN, 0.2)
    pos = np.asarray([1, 4])                                        # a positive of weight 0 is still drawn as a positive
    # a call makes 2 deg = 4 draws: 50,000 calls, each under a pass counter of its own
    got = np.concatenate([P.mixture_draws(w, pos, seed=7, pas=block, user=5) for block in range(N_DRAWS // 4)])
    assert len(got) == N_DRAWS
    pn = 0.8 * w / float(w.sum())
    pn[pos] += 0.2 / len(pos)
    _within(np.bincount(got, minlength=7).astype(np.float64), pn, N_DRAWS)


def test_the_weights_subtract_the_maximum_and_floor():
    z = np.asarray([500.0, 499.0, 300.0])                           # np.exp(500) overflows; the shifted form does not
    w = P.weights(z, 1.0)
    assert w.tolist() == [2 ** 31, int(np.floor(np.exp(-1.0) * 2 ** 31)), 0]
    assert P.weights(np.zeros(5), 0.2).tolist() == [2 ** 31] * 5
    assert P.weights([0.0, -21.4], 1.0)[1] == 1 and P.weights([0.0, -21.6], 1.0)[1] == 0      # 2^-31 = exp(-21.49)


# ------------------------------------------------------------------ the plugin on the host
def test_find_recommender_resolves_irgan():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import AbstractRecommender
    cls = find_recommender("IRGAN")
    assert cls.__module__ == "neurec_amd.model.general_recommender.IRGAN" and issubclass(cls, AbstractRecommender)
    doc = sys.modules[cls.__module__].__doc__
    assert "As the reference" in doc and "Deviations" in doc
    for point in ("any(", "B times", "not excluded", "0.2", "maximum logit", "2^-31", "fixed seed", "latin", "absent"):
        assert point in doc, point
    keys = re.findall(r'conf\["(\w+)"\]', inspect.getsource(cls.__init__))
    assert keys == ["factors_num", "lr", "g_reg", "d_reg", "epochs", "g_epoch", "d_epoch", "batch_size", "d_tau", "topk",
                    "pretrain_file"]
    assert list(inspect.signature(cls.__init__).parameters) == ["self", "sess", "dataset", "conf"]


def test_the_defaults_row_equals_the_properties_file(tmp_path):
    from neurec_amd import defaults
    ref = configparser.ConfigParser()
    ref.optionxform = str
    assert ref.read(os.path.join(GOLDEN, "neurec_conf", "conf", "IRGAN.properties"))
    want = dict(ref["hyperparameters"])
    assert dict(defaults.MODELS["IRGAN"]) == want and [k for k, _ in defaults.MODELS["IRGAN"]] == list(want)
    assert want["d_reg"] == "0.1/16"
    path = defaults.write_default_configs(str(tmp_path))
    from neurec_amd.util.configurator import Configurator
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=IRGAN"])
    finally:
        os.chdir(cwd)
    assert (conf["factors_num"], conf["batch_size"], conf["d_reg"], conf["d_tau"], conf["lr"]) == (20, 32, 0.1 / 16, 0.2, 0.001)
    assert conf["pretrain_file"] == "dataset/ml100k_saved_model.pkl"


class _Engine:
    def __init__(self, size):
        self.calls, self.size = [], size

    def d_pass_size(self):
        return self.size

    def d_pass(self, order, loss_out=None, data=None):
        self.calls.append(("d", np.asarray(order).copy()))

    def g_pass(self):
        self.calls.append(("g", None))


def _bare(lines):
    from neurec_amd.model.general_recommender.IRGAN import IRGAN
    model = IRGAN.__new__(IRGAN)
    model.logger = type("L", (), {"info": staticmethod(lambda m: lines.append(str(m)))})()
    model.evaluator = type("E", (), {"evaluate": staticmethod(lambda m: "recorded")})()
    return model


@pytest.mark.parametrize("case", sorted(P.CASES))
def test_the_plugin_runs_the_recorded_schedule_and_logs_its_lines(golden, case):
    """train_model() on a counting engine against the reference's recorded run: the same sequence of passes, every D
    pass one permutation of the pass's triples walked in batches of batch_size, one log line per G pass"""
    g = golden
    g_reg, d_reg, d_tau, d_epoch, g_epoch = P.CASES[case]
    lines = []
    model = _bare(lines)
    size = int(g["%s_pass_ptr" % case][1])
    model.engine = _Engine(size)
    model.epochs, model.d_epoch, model.g_epoch, model.batch_size = 2, d_epoch, g_epoch, P.BATCH
    model.train_model()
    calls = model.engine.calls
    assert "".join(k for k, _ in calls) == ("d" * d_epoch + "g" * g_epoch) * 2
    orders = [o for k, o in calls if k == "d"]
    assert all(sorted(o.tolist()) == list(range(size)) and o.dtype == np.int32 for o in orders)
    assert not np.array_equal(orders[0], orders[1])                  # reshuffled per pass
    assert lines == g["%s_log" % case].tolist()[2:] == ["recorded"] * (2 * g_epoch)
    model.engine = _Engine(0)                                        # no train user: empty passes, the same lines
    lines[:] = []
    model.train_model()
    assert [len(o) for k, o in model.engine.calls if k == "d"] == [0] * (2 * d_epoch) and len(lines) == 2 * g_epoch


def test_the_any_rule_of_the_engine_is_the_reference_s(golden):
    from neurec_amd.irgan import train_users_of
    g = golden
    assert train_users_of(g["indptr"], g["indices"]).tolist() == P.train_users(g["indptr"], g["indices"])
    indptr, indices = np.asarray([0, 0, 1, 3, 4, 4]), np.asarray([0, 0, 5, 7])
    assert train_users_of(indptr, indices).tolist() == [2, 3] == P.train_users(indptr, indices)
    assert train_users_of(np.asarray([0]), np.zeros(0, np.int32)).tolist() == []


def test_the_refusals_name_the_key_and_the_range(monkeypatch):
    from neurec_amd.irgan import check_config
    ok = dict(factors_num=20, batch_size=32, d_tau=0.2, g_reg=0.0, d_reg=0.1 / 16, lr=0.001)
    check_config(**ok)
    check_config(**dict(ok, factors_num=128, batch_size=1024, g_reg=0.5))
    check_config(**dict(ok, factors_num=1, batch_size=1))
    for change, exc, text in ((dict(factors_num=0), NotImplementedError, r"factors_num=0 is not supported \(1 to 128\)"),
                              (dict(factors_num=129), NotImplementedError, r"factors_num=129 is not supported \(1 to 128\)"),
                              (dict(batch_size=0), NotImplementedError, r"batch_size=0 is not supported \(1 to 1024\)"),
                              (dict(batch_size=1025), NotImplementedError, r"batch_size=1025 is not supported"),
                              (dict(d_tau=0.0), ValueError, r"d_tau=0.0 is not supported \(above 0\)"),
                              (dict(d_tau=-1), ValueError, r"d_tau=-1 is not supported"),
                              (dict(g_reg=-0.1), ValueError, r"g_reg=-0.1 is not supported \(0 or more\)"),
                              (dict(d_reg=-1e-3), ValueError, r"d_reg=-0.001 is not supported \(0 or more\)"),
                              (dict(lr=0), ValueError, r"lr=0 is not supported \(above 0\)")):
        with pytest.raises(exc, match=text):
            check_config(**dict(ok, **change))
    from neurec_amd import parallel
    model = _bare([])
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)
    with pytest.raises(NotImplementedError, match="IRGAN runs on one GPU"):
        model.build_graph()


def test_the_c_entries_refuse_by_name():
    import ctypes as C
    from neurec_amd import _lib
    floats = C.c_size_t(0)
    with pytest.raises(NotImplementedError, match=r"irgan_workspace: d=129 is not supported \(1 to 128\)"):
        _lib.call("nrhip_irgan_workspace", 100, 129, 32, C.byref(floats))
    with pytest.raises(NotImplementedError, match=r"a batch of 1025 pairs is not supported \(up to 1024\)"):
        _lib.call("nrhip_irgan_workspace", 100, 20, 1025, C.byref(floats))
    _lib.call("nrhip_irgan_workspace", 40981, 20, 1024, C.byref(floats))
    assert floats.value >= 2 * 1024 * 20 + 1024 + 161 + 101 * 20
    with pytest.raises(ValueError, match="irgan_d_pass: null argument block"):
        _lib.call("nrhip_irgan_d_pass", None, None, None, None, None, 0, 1, None, None)
    with pytest.raises(ValueError, match="irgan_weights: bad arguments"):
        _lib.call("nrhip_irgan_weights", None, 4, 1, 4, 0.0, None)
    _lib.call("nrhip_irgan_weights", None, 4, 0, 4, 0.2, None)                          # no rows: nothing to do
    a = _lib.IrganArgs()
    a.n_items, a.d, a.max_batch = 67, 5, 1024
    _lib.call("nrhip_irgan_g_pass", C.byref(a), None, 0, None, 0, None)                 # no train users
    with pytest.raises(ValueError, match="irgan_g_pass: null argument"):
        _lib.call("nrhip_irgan_g_pass", C.byref(a), None, 1, None, 0, None)


# ------------------------------------------------------------------ the pretrain_file branches
def test_the_pretrain_file_branches(tmp_path):
    from neurec_amd.model.general_recommender.IRGAN import initial_tables
    lines = []
    model = _bare(lines)
    model.pretrain_file = str(tmp_path / "absent.pkl")
    assert model.load_pretrain() is None
    assert len(lines) == 1 and "does not exist" in lines[0] and "absent.pkl" in lines[0]
    T = initial_tables(7, 9, 4, None)
    assert list(T) == list(P.NAMES) and T["g_P"].shape == (7, 4) and T["g_Q"].shape == (9, 4)
    assert not T["g_b"].any() and not T["d_b"].any() and all(v.dtype == np.float32 for v in T.values())
    for k in ("g_P", "g_Q", "d_P", "d_Q"):
        assert np.abs(T[k]).max() <= 0.05 and np.abs(T[k]).max() > 0.03
    assert all(np.array_equal(v, initial_tables(7, 9, 4, None)[k]) for k, v in T.items())     # a fixed seed
    rs = np.random.RandomState(1)
    held = [rs.randn(7, 4).astype(np.float32), rs.randn(9, 4).astype(np.float32), rs.randn(9).astype(np.float32)]
    path = tmp_path / "g.pkl"
    with open(str(path), "wb") as f:
        pickle.dump(held, f, protocol=2)
    model.pretrain_file, lines[:] = str(path), []
    got = model.load_pretrain()
    assert lines == [] and all(np.array_equal(a, b) for a, b in zip(got, held))
    T2 = initial_tables(7, 9, 4, got)
    assert np.array_equal(T2["g_P"], held[0]) and np.array_equal(T2["g_b"], held[2])
    assert np.array_equal(T2["d_P"], T["d_P"]) and np.array_equal(T2["d_Q"], T["d_Q"])       # D does not depend on the file
    with pytest.raises(ValueError, match=r"pretrain_file holds P \[7, 4\], Q \[9, 4\], b \[9\]; \[8, 4\]"):
        initial_tables(8, 9, 4, got)
    with pytest.raises(ValueError, match=r"must hold \[P, Q, b\], got 2 entries"):
        initial_tables(7, 9, 4, got[:2])
