"""CDAE without a GPU: the restated generators, the batch layout, the once-per-batch regulariser against a
finite-difference gradient of the restated loss, the plugin's config keys, defaults and refusals."""
import configparser
import inspect
import os
import re
import sys

import numpy as np
import pytest

import cdae_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _toy():
    I = 41
    rows = R.random_rows([3, 1, 7, 12, 5, 2], I, 3)
    return (I,) + R.csr_of(rows, I)


# ------------------------------------------------------------------ the reference's trace
@pytest.fixture(scope="module")
def golden():
    from conftest import load_golden
    return load_golden("tfgraph_cdae")


def _ragged(flat, ptr):
    return [flat[ptr[k]:ptr[k + 1]] for k in range(len(ptr) - 1)]


def case_init(g, case):
    U, I = (int(x) for x in g["shape"])
    d = R.CASES[R.EPOCH_CASE if case == "epoch" else case][4]
    return R.init_tables(U, I, d, seed=int(g[case + "_init_seed"]))


def case_steps(g, case):
    """(users, negatives per slot, uniforms) of every recorded step"""
    for s in range(int(g["steps"])):
        yield g[case + "_users"][s], _ragged(g["%s_neg_%d" % (case, s)], g["%s_negptr_%d" % (case, s)]), \
            g["%s_unif_%d" % (case, s)]


def epoch_steps(g):
    """the same for the recorded train_model() epoch, read back from what the class fed"""
    for s in range(int(g["epoch_steps"])):
        users, items = g["epoch_users_%d" % s], g["epoch_items_%d" % s]
        labels, idx = g["epoch_labels_%d" % s], g["epoch_idx_%d" % s]
        yield users, [items[(idx == k) & (labels == 0)] for k in range(len(users))], g["epoch_unif_%d" % s]


def golden_table(g, case, name, s, init):
    return init[name].astype(np.float64) + g["%s_f64_%s" % (case, name)][s]


def keep_prob_of(dropout):
    return float(np.float32(1.0) - np.float32(dropout))


def _close(got, want, bar, what):
    """the trace's rule: 4 x the reference's own f32-to-f64 distance plus 1e-5 max|want|"""
    err = np.abs(np.asarray(got, np.float64) - want).max(initial=0)
    assert np.shape(got) == np.shape(want) and err <= 4 * bar + 1e-5 * np.abs(want).max(initial=0), (what, err, bar)


def _follow(g, case, steps, hyper_case):
    act, loss, reg, dropout, d = R.CASES[hyper_case]
    indptr, indices = g["indptr"], g["indices"]
    init = case_init(g, case)
    adam = R.Adam(init, float(g["lr"]))
    losses = []
    for users, negs, unif in steps:
        b = R.build_batch(indptr, indices, users, negs)
        (a, r), G = R.gradients(adam.T, b, R.keep_of(unif, dropout), keep_prob_of(dropout), reg, act, loss)
        losses.append(a + r)
        adam.apply(G)
        yield b, losses[-1], adam.T, init


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_the_restatement_follows_the_reference_trace(golden, case):
    """every variable after every step and each step's loss, and predict() after the last step, against the float64
    run of the reference's own class under the trace's rule"""
    g = golden
    assert sorted(R.CASES) == g["cases"].tolist()
    dropout = R.CASES[case][3]
    for s, (b, loss, T, init) in enumerate(_follow(g, case, case_steps(g, case), case)):
        l64, l32 = g[case + "_loss_f64"][s], g[case + "_loss_f32"][s]
        _close([loss], [l64], abs(l32 - l64), "%s step %d loss" % (case, s + 1))
        for name in R.TABLES:
            _close(T[name], golden_table(g, case, name, s, init), g["%s_gap_%s" % (case, name)][s],
                   "%s step %d %s" % (case, s + 1, name))
    users = g["predict_users"]
    keep = R.keep_of(g["predict_%s_unif" % case], dropout)
    got, _ = R.predict(T, g["indptr"], g["indices"], users, keep, keep_prob_of(dropout), R.CASES[case][0])
    f32, f64 = g["predict_%s_f32" % case], g["predict_%s_f64" % case]
    assert f64.shape == (27, 131)
    _close(got, f64, np.abs(f32 - f64).max(), "predict %s" % case)


def test_the_trace_s_batches_hold_what_the_issue_names(golden):
    """in every recorded step: a repeated user, an item that is positive for one user and negative for another, and —
    where the case has dropout — a user all of whose entries are dropped"""
    g = golden
    for case in sorted(R.CASES):
        dropout = R.CASES[case][3]
        for users, negs, unif in case_steps(g, case):
            b = R.build_batch(g["indptr"], g["indices"], users, negs)
            assert len(set(users.tolist())) < len(users)
            assert set(b["items"][b["labels"] == 1].tolist()) & set(b["items"][b["labels"] == 0].tolist())
            keep = R.keep_of(unif, dropout)
            dropped = [not keep[b["entry_ptr"][k]:b["entry_ptr"][k + 1]].any() for k in range(len(users))]
            assert any(dropped) == (dropout > 0) and keep.any()


def test_the_recorded_epoch_is_laid_out_and_ends_as_restated(golden):
    """what train_model() itself fed — items, labels, remap_idx and the sparse indices of every batch — is
    build_batch of its users and negatives; the restated epoch ends at the reference's tables"""
    g = golden
    users_seen = []
    for s, (users, negs, unif) in enumerate(epoch_steps(g)):
        b = R.build_batch(g["indptr"], g["indices"], users, negs)
        assert np.array_equal(b["items"], g["epoch_items_%d" % s]) and np.array_equal(b["slot"], g["epoch_idx_%d" % s])
        assert np.array_equal(b["labels"], g["epoch_labels_%d" % s])
        rows = np.repeat(np.arange(len(users)), np.diff(b["entry_ptr"]))
        assert np.array_equal(np.stack([rows, b["in_items"]], axis=1), g["epoch_spidx_%d" % s])
        assert len(unif) == len(b["items"])
        users_seen += users.tolist()
    deg = np.diff(g["indptr"])
    assert sorted(users_seen) == np.flatnonzero(deg > 0).tolist()           # every user with a train item, once
    for _, _, T, init in _follow(g, "epoch", epoch_steps(g), R.EPOCH_CASE):
        pass
    for name in R.TABLES:
        _close(T[name], golden_table(g, "epoch", name, 0, init), g["epoch_gap_" + name][0], "epoch end " + name)


# ------------------------------------------------------------------ the generators
def test_the_draws_are_deterministic_and_do_not_depend_on_the_batch():
    I, indptr, indices, _ = _toy()
    a = R.negatives(5, [0, 2, 3], indptr, indices, I, 4)
    b = R.negatives(5, [3, 3, 1, 0, 2], indptr, indices, I, 4)
    assert all(np.array_equal(x, y) for x, y in zip(a, [b[3], b[4], b[0]]))
    assert np.array_equal(b[0], b[1])                                     # a repeated user draws the same
    assert not np.array_equal(a[2], R.negatives(6, [3], indptr, indices, I, 4)[0])
    row = indices[indptr[3]:indptr[4]]
    d = R.draws(5, 3, row, I, 48)
    assert np.array_equal(d[:10], R.draws(5, 3, row, I, 10))              # a prefix: draw q is keyed by q alone
    assert d.min() >= 0 and d.max() < I and not np.intersect1d(d, row).size
    assert np.array_equal(a[2], np.unique(d))


def test_draws_of_a_user_who_holds_almost_every_item():
    """63 rejections in a row are rare but the closed form behind them must name an allowed item; a full row draws
    nothing"""
    I = 50
    row = np.delete(np.arange(I), [7, 31])
    d = R.draws(1, 0, row, I, 400)
    assert set(d.tolist()) == {7, 31}
    assert (R.draws(1, 0, np.arange(I), I, 5) == -1).all()


def test_the_mask_generator_is_deterministic_and_fair():
    """the seed the GPU test uses: over 20,000 entries at keep 0.5 the kept share is within five binomial standard
    deviations (5 sqrt(0.25 / 20000) = 0.018) of 0.5"""
    m = R.mask(2018 + 1, 1, 20000, 0.5)
    assert abs(m.mean() - 0.5) <= 0.018
    assert np.array_equal(m[:300], R.mask(2018 + 1, 1, 300, 0.5))
    assert not np.array_equal(m[:300], R.mask(2018 + 1, 2, 300, 0.5))
    assert R.mask(3, 0, 500, 1.0).all()


# ------------------------------------------------------------------ the batch
def test_the_batch_layout_is_the_reference_s():
    """positives ascending then negatives ascending per slot; the input row-major with ascending columns"""
    I, indptr, indices, _ = _toy()
    users = [2, 0, 2]
    negs = R.negatives(9, users, indptr, indices, I, 2)
    b = R.build_batch(indptr, indices, users, negs)
    lo, hi = b["entry_ptr"][0], b["entry_ptr"][1]
    row = indices[indptr[2]:indptr[3]]
    assert np.array_equal(b["items"][lo:hi], np.r_[row, negs[0]]) and b["labels"][lo:hi].sum() == len(row)
    assert np.array_equal(b["in_items"][lo:hi], np.sort(np.r_[row, negs[0]]))
    assert np.array_equal(b["in_items"][b["in_pos"]], b["items"])
    assert np.array_equal(b["slot"], np.repeat([0, 1, 2], np.diff(b["entry_ptr"])))


# ------------------------------------------------------------------ the regulariser
@pytest.mark.parametrize("act,loss", [("sigmoid", "sigmoid_cross_entropy"), ("identity", "square")])
def test_the_gradient_is_the_finite_difference_of_the_loss(act, loss):
    """every variable's gradient against central differences of data term + regulariser in float64.  The batch holds a
    repeated user and items that several users hold, as a positive for one and a negative for another: an item row
    regularised per occurrence, or a user row regularised once, would miss by reg * row"""
    I, indptr, indices, _ = _toy()
    U, d, reg, keep_prob = 6, 5, 0.3, 0.5
    users = [3, 2, 3, 4]
    negs = R.negatives(4, users, indptr, indices, I, 2)
    b = R.build_batch(indptr, indices, users, negs)
    pos = set(b["items"][b["labels"] == 1].tolist())
    neg = set(b["items"][b["labels"] == 0].tolist())
    assert pos & neg and len(np.unique(b["items"])) < len(b["items"])
    keep = (np.random.RandomState(2).rand(len(b["items"])) < keep_prob).astype(np.uint8)
    T = {k: v.astype(np.float64) for k, v in R.init_tables(U, I, d, 7, scale=0.5).items()}
    _, G = R.gradients(T, b, keep, keep_prob, reg, act, loss)

    def total(Tx):
        a, r, _ = R.loss_terms(Tx, b, keep, keep_prob, reg, act, loss)
        return a + r
    rs = np.random.RandomState(3)
    eps = 1e-6
    for name in R.TABLES:
        flat = T[name].reshape(-1)
        for j in rs.choice(flat.size, min(flat.size, 25), replace=False):
            up, dn = {k: v.copy() for k, v in T.items()}, {k: v.copy() for k, v in T.items()}
            up[name].reshape(-1)[j] += eps
            dn[name].reshape(-1)[j] -= eps
            fd = (total(up) - total(dn)) / (2 * eps)
            assert abs(fd - G[name].reshape(-1)[j]) <= 1e-6 * max(1.0, abs(fd)), (name, j, fd, G[name].reshape(-1)[j])
    shared = sorted(pos & neg)[0]
    occ = int((b["items"] == shared).sum())
    assert occ >= 2
    # the item's regulariser gradient is reg * row once: with the data terms removed (reg alone) it shows directly
    _, G0 = R.gradients(T, b, keep, keep_prob, 0.0, act, loss)
    assert np.allclose(G["de_embeddings"][shared] - G0["de_embeddings"][shared], reg * T["de_embeddings"][shared])
    assert np.allclose(G["user_embeddings"][3] - G0["user_embeddings"][3], 2 * reg * T["user_embeddings"][3])


# ------------------------------------------------------------------ the plugin on the host
def test_find_recommender_resolves_cdae():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import AbstractRecommender
    cls = find_recommender("CDAE")
    assert cls.__module__ == "neurec_amd.model.general_recommender.CDAE" and issubclass(cls, AbstractRecommender)
    doc = sys.modules[cls.__module__].__doc__
    assert "As the reference" in doc and "Deviations" in doc
    keys = re.findall(r'config\["(\w+)"\]', inspect.getsource(cls.__init__))
    assert keys == ["hidden_dim", "lr", "reg", "dropout", "loss_func", "num_neg", "epochs", "batch_size", "hidden_act"]


def test_the_defaults_row_equals_the_properties_file(tmp_path):
    from neurec_amd import defaults
    ref = configparser.ConfigParser()
    ref.optionxform = str
    assert ref.read(os.path.join(GOLDEN, "neurec_conf", "conf", "CDAE.properties"))
    want = dict(ref["hyperparameters"])
    assert list(want) == ["lr", "reg", "hidden_dim", "dropout", "num_neg", "epochs", "batch_size", "hidden_act",
                          "loss_func"]
    assert dict(defaults.MODELS["CDAE"]) == want and [k for k, _ in defaults.MODELS["CDAE"]] == list(want)
    path = defaults.write_default_configs(str(tmp_path))
    from neurec_amd.util.configurator import Configurator
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=CDAE"])
    finally:
        os.chdir(cwd)
    assert (conf["lr"], conf["reg"], conf["hidden_dim"], conf["dropout"], conf["num_neg"], conf["epochs"]) == \
        (0.001, 0.001, 64, 0.5, 5, 5000)
    assert (conf["batch_size"], conf["hidden_act"], conf["loss_func"]) == (32, "sigmoid", "sigmoid_cross_entropy")


def test_the_value_errors_and_the_refusals():
    from neurec_amd.cdae import check_config
    assert check_config("sigmoid", "square", 5, 64) == (1, 1) and check_config("identity", "sigmoid_cross_entropy", 1, 1) == (0, 0)
    with pytest.raises(ValueError, match=r"^hidden activate function relu is invalid\.$"):
        check_config("relu", "square", 5, 64)
    with pytest.raises(ValueError, match=r"^log_loss is an invalid loss function\.$"):
        check_config("sigmoid", "log_loss", 5, 64)
    with pytest.raises(ValueError, match=r"CDAE: num_neg=0 is not supported"):
        check_config("sigmoid", "square", 0, 64)
    for d in (0, 129):
        with pytest.raises(NotImplementedError, match=r"CDAE: hidden_dim=%d is not supported \(1 to 128\)" % d):
            check_config("sigmoid", "square", 5, d)


def _plugin(**attrs):
    from neurec_amd.model.general_recommender.CDAE import CDAE
    model = CDAE.__new__(CDAE)
    base = dict(hidden_act="sigmoid", loss_func="square", num_neg=5, emb_size=64)
    base.update(attrs)
    for k, v in base.items():
        setattr(model, k, v)
    return model


def test_the_plugin_refuses_by_name(monkeypatch):
    with pytest.raises(ValueError, match="tanh is an invalid loss function"):
        _plugin(loss_func="tanh").build_graph()
    with pytest.raises(ValueError, match="num_neg=0 is not supported"):
        _plugin(num_neg=0).build_graph()
    with pytest.raises(NotImplementedError, match="hidden_dim=200 is not supported"):
        _plugin(emb_size=200).build_graph()
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)
    with pytest.raises(NotImplementedError, match="CDAE runs on one GPU"):
        _plugin().build_graph()


def test_the_c_entries_refuse_by_name():
    import ctypes as C
    from neurec_amd import _lib
    a = _lib.CdaeStepArgs()
    a.d, a.batch, a.keep_prob, a.n_users, a.n_items = 129, 1, 0.5, 3, 5
    with pytest.raises(NotImplementedError, match=r"hidden_dim 129 outside 1\.\.128"):
        _lib.call("nrhip_cdae_step", C.byref(a), None)
    a.d, a.batch = 8, 1025
    with pytest.raises(NotImplementedError, match=r"batch 1025 outside 0\.\.1024"):
        _lib.call("nrhip_cdae_step", C.byref(a), None)
    a.batch, a.act = 1, 2
    with pytest.raises(ValueError, match="unknown activation 2"):
        _lib.call("nrhip_cdae_step", C.byref(a), None)
    a.act, a.loss_kind = 1, 5
    with pytest.raises(ValueError, match="unknown pointwise loss 5"):
        _lib.call("nrhip_cdae_step", C.byref(a), None)
    a.loss_kind, a.keep_prob = 0, 0.0
    with pytest.raises(ValueError, match=r"keep_prob 0 outside \(0, 1\]"):
        _lib.call("nrhip_cdae_step", C.byref(a), None)
    a.keep_prob = 0.5
    with pytest.raises(ValueError, match="null pointer argument"):
        _lib.call("nrhip_cdae_step", C.byref(a), None)
    b = _lib.CdaeBatchArgs()
    b.batch, b.num_neg, b.n_items = 2, 0, 5
    with pytest.raises(ValueError, match="num_neg must be at least 1, got 0"):
        _lib.call("nrhip_cdae_batch", C.byref(b), None)
    b.num_neg, b.batch = 1, 1025
    with pytest.raises(NotImplementedError, match=r"batch 1025 outside 0\.\.1024"):
        _lib.call("nrhip_cdae_batch", C.byref(b), None)
    b.batch = 0
    _lib.call("nrhip_cdae_batch", C.byref(b), None)                       # an empty batch launches nothing
