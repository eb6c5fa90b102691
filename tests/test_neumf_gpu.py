"""NeuMF and MLP on the GPU (csrc/neumf.hip through neurec_amd/neumf.py): every step of the reference classes' trace, the
recorded epoch, predict() in both modes, the step's gradients and the all-items scorer on the edge shapes against the
float64 restatement, determinism, empty work, ids outside the tables and the drop-in runs through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import neumf_restatement as P
from neumf_restatement import CASES
from test_neumf_cpu import case_feeds, case_init, golden_table
from test_gru4rec_gpu import _close, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_neumf")


def _engine(tab, layers, max_batch, lr=0.001, reg_mf=0.0, reg_mlp=0.0, loss="cross_entropy", learner="adam"):
    from neurec_amd.neumf import NeuMFEngine
    return NeuMFEngine(tab, layers, lr, reg_mf, reg_mlp, max_batch, loss=loss, learner=learner)


def _case_engine(g, case, init=None, batch=None):
    _, layers, d, loss, learner, reg_mf, reg_mlp, _ = CASES[case]
    init = case_init(g, case) if init is None else init
    return _engine(init, layers, int(g["batch_step"]) if batch is None else batch, float(g["lr"]), reg_mf, reg_mlp, loss,
                   learner), init


def _tables(eng):
    return {k: t.cpu().numpy() for k, t in eng.tables().items()}


def _loss2(eng):
    import torch
    return torch.zeros(2, device=eng.T["mlp_embedding_user"].device)


def _clean(eng):
    for name, G in eng.G.items():
        assert not G.any().item(), name
    for name, flag in eng.flag.items():
        assert flag is None or not flag.any().item(), name


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Every variable after every step, and each step's loss, against the f64 trace: within 4x the reference's own
    f32-to-f64 distance of that step and tensor (read from the golden) plus 1e-5 max|want|.  The gradient buffers and
    the row flags are zero again afterwards."""
    g = golden
    eng, init = _case_engine(g, case)
    _, layers, d = CASES[case][:3]
    assert list(eng.tables()) == P.names(layers, d)
    loss2 = _loss2(eng)
    for s, (users, items, labels) in enumerate(case_feeds(g, case)):
        eng.step(users, items, labels, loss2)
        l64, l32 = float(g[case + "_loss_f64"][s]), float(g[case + "_loss_f32"][s])
        _close(np.asarray([loss2.sum().item()]), np.asarray([l64]), abs(l32 - l64), "%s step %d loss" % (case, s + 1))
        for name, got in _tables(eng).items():
            _close(got, golden_table(g, case, name, s, init)[0], float(g["%s_gap_%s" % (case, name)][s]),
                   "%s step %d %s" % (case, s + 1, name))
        _clean(eng)
    assert eng.t == CASES[case][7]


def test_the_recorded_epoch_ends_at_the_reference_tables(golden):
    """train_model()'s epoch of the golden, batch by batch in the order the class was fed, the last batch cut to its
    true size; the end tables under the trace's rule"""
    import torch
    g = golden
    eng, init = _case_engine(g, P.EPOCH_CASE, case_init(g, "epoch"), int(g["batch_epoch"]))
    dev = eng.T["mlp_embedding_user"].device
    users = torch.from_numpy(g["epoch_users"]).to(dev)
    items = torch.from_numpy(g["epoch_items"]).to(dev)
    labels = torch.from_numpy(g["epoch_labels"]).to(dev)
    rows = g["epoch_rows"]
    losses = torch.zeros((len(rows), 2), device=dev)
    for s, n in enumerate(rows):
        eng.step(users[s, :n], items[s, :n], labels[s, :n], losses[s])
    assert eng.t == len(rows) and np.isfinite(losses.cpu().numpy()).all()
    for name, got in _tables(eng).items():
        _close(got, golden_table(g, "epoch", name, 0, init)[0], float(g["epoch_gap_" + name][0]), "epoch end %s" % name)


@pytest.mark.parametrize("case", P.PREDICT_CASES)
def test_predict_matches_the_reference(golden, case):
    """predict(), full and candidate mode, after the case's last step, under the trace's rule"""
    from neurec_amd.model.general_recommender.NeuMF import predict_pairs
    g = golden
    eng, _ = _case_engine(g, case)
    loss2 = _loss2(eng)
    for users, items, labels in case_feeds(g, case):
        eng.step(users, items, labels, loss2)
    users, cand = g["predict_users"], g["predict_cand"]
    got = predict_pairs(eng, users, None)
    assert got.is_cuda and tuple(got.shape) == (27, 131)
    f32, f64 = g["predict_%s_f32" % case], g["predict_%s_f64" % case]
    _close(got.cpu().numpy(), f64, np.abs(f32 - f64).max(), "predict %s" % case)
    got_c = predict_pairs(eng, users, [list(c) for c in cand])
    assert len(got_c) == 27 and all(isinstance(r, np.ndarray) and r.shape == (3,) for r in got_c)
    f32, f64 = g["predict_cand_%s_f32" % case], g["predict_cand_%s_f64" % case]
    _close(np.stack(got_c), f64, np.abs(f32 - f64).max(), "predict %s, candidates" % case)


# ------------------------------------------------------------------ the step's gradients on the edge shapes
def _batch(U, I, B, seed, pattern=None):
    rs = np.random.RandomState(seed)
    users, items = rs.randint(0, U, B).astype(np.int32), rs.randint(0, I, B).astype(np.int32)
    if pattern == "one user":
        users[:] = users[0]
    if pattern == "one item":
        items[:] = items[0]
    return users, items, rs.randint(0, 2, B).astype(np.float32)


WIDTH_CASES = [([1], 2), ([2, 1], 3), ([33, 17, 9, 5], 5), ([128, 128, 128, 128], 128), ([8, 4], 0), ([9, 4], 1),
               ([64, 32, 16], 17)]
# (layers, embedding_size, batch, pattern, loss)
GRADIENT_CASES = [([64, 32, 16], 16, 1, None, "cross_entropy"), ([64, 32, 16], 16, 257, None, "cross_entropy"),
                  ([7, 5, 3], 3, 257, None, "square"), ([64, 32, 16], 16, 40, "one user", "square"),
                  ([64, 32, 16], 16, 40, "one item", "cross_entropy"),
                  ([128, 128, 128, 128], 128, 257, None, "cross_entropy")] + \
                 [(layers, d, 37, None, "square") for layers, d in WIDTH_CASES]


def _check_gradients(tab, layers, users, items, labels, loss, reg_mf, reg_mlp, max_batch):
    eng = _engine(tab, layers, max_batch, reg_mf=reg_mf, reg_mlp=reg_mlp, loss=loss)
    loss2 = _loss2(eng)
    eng.gradients(users, items, labels, loss2)
    (term, reg), want = P.gradients(tab, users, items, labels, layers, loss, reg_mf, reg_mlp)
    got2 = loss2.cpu().numpy()
    assert abs(got2[0] - term) <= 1e-5 * max(abs(term), 1e-30) and abs(got2[1] - reg) <= 1e-5 * abs(reg), (got2, term, reg)
    for name, w in want.items():
        got = eng.G[name].cpu().numpy()
        err = np.abs(got - w).max(initial=0)
        print("%s: err %.3g of max %.3g" % (name, err, np.abs(w).max(initial=0)))
        assert got.shape == w.shape and err <= 1e-5 * np.abs(w).max(initial=0), (name, err, np.abs(w).max(initial=0))
    assert eng.t == 0
    return eng, want


@pytest.mark.parametrize("layers,d,B,pattern,loss", GRADIENT_CASES)
def test_gradients_equal_the_restatement(layers, d, B, pattern, loss):
    """every gradient at 1e-5 max|want| per tensor: fp32 sums of a few hundred terms of one sign-mixed scale sit two
    orders below it, a dropped or doubled term two orders above"""
    U, I = 23, 29
    tab = P.init_tables(U, I, d, layers, seed=len(layers) * 131 + d)
    users, items, labels = _batch(U, I, B, B + d, pattern)
    eng, want = _check_gradients(tab, layers, users, items, labels, loss, 0.03 if d else 0.0, 0.05, max(B, 2))
    for name in ("mlp_embedding_user", "mlp_embedding_item"):
        ids = users if name.endswith("user") else items
        if eng.flag[name] is not None:
            assert np.array_equal(np.flatnonzero(eng.flag[name].cpu().numpy()), np.unique(ids))


def test_gradients_where_a_whole_layer_is_dead():
    """every pre-activation of the second layer negative: no gradient passes it, the GMF branch still learns"""
    U, I, layers, d, B = 23, 29, [16, 8, 4], 6, 33
    tab = P.init_tables(U, I, d, layers, seed=77)
    tab["bias1"][:] = -100.0
    users, items, labels = _batch(U, I, B, 78)
    _, _, pre = P.forward(tab, users, items, layers)
    assert (pre[1] < 0).all()
    _, want = _check_gradients(tab, layers, users, items, labels, "square", 0.0, 0.0, B)
    assert not want["kernel0"].any() and not want["kernel1"].any() and not want["mlp_embedding_user"].any()
    assert want["bias2"].any() and want["mf_embedding_user"].any()


def test_gradients_at_a_pre_activation_of_exactly_zero():
    """the second layer's kernel and bias are zero: relu passes nothing at a pre-activation of 0"""
    from test_neumf_cpu import zero_pre_activation_point
    tab, layers, (users, items, labels) = zero_pre_activation_point()
    _, want = _check_gradients(tab, layers, users, items, labels, "square", 0.0, 0.0, 16)
    assert not want["kernel1"].any() and not want["kernel0"].any() and want["bias2"].any()


def test_the_learners_flags_mark_the_batch_s_rows():
    U, I, layers, d = 23, 29, [8, 4], 3
    tab = P.init_tables(U, I, d, layers, seed=9)
    eng = _engine(tab, layers, 16, learner="gd", loss="square")
    users, items, labels = _batch(U, I, 16, 10)
    eng.gradients(users, items, labels, _loss2(eng))
    for name, flag in eng.flag.items():
        ids = users if name.endswith("user") else items
        assert np.array_equal(np.flatnonzero(flag.cpu().numpy()), np.unique(ids)), name
    eng.apply()
    _clean(eng)


# ------------------------------------------------------------------ the all-items scorer
def _check_scores(tab, layers, users, I, guard=False):
    import torch
    eng = _engine(tab, layers, 8)
    want = P.scores(tab, users, layers)
    n = len(users)
    if guard:
        out = torch.full((n + 1, I + 3), -7.5, device=eng.T["mlp_embedding_user"].device)
        got = eng.score(users, out=out)
        whole = out.cpu().numpy()
        assert (whole[n:] == -7.5).all() and (whole[:, I:] == -7.5).all()
    else:
        got = eng.score(users)
    assert got.is_cuda and tuple(got.shape) == (n, I)
    got = got.cpu().numpy()
    err = np.abs(got - want).max(initial=0)
    print("scores: err %.3g of max %.3g" % (err, np.abs(want).max(initial=0)))
    assert err <= 1e-5 * np.abs(want).max(initial=0), (err, np.abs(want).max(initial=0))
    return eng, got


@pytest.mark.parametrize("I", [1, 31, 33, 131])
@pytest.mark.parametrize("n", [1, 5, 65])
def test_scores_on_partial_tiles(I, n):
    """item tiles of 32, user tiles of 32: I = 33 with n = 65 leaves one item and one user in the last tiles at once; the
    guard row and columns of the output stay as they were"""
    U, layers, d = 70, [64, 32, 16], 16
    tab = P.init_tables(U, I, d, layers, seed=I + n)
    users = np.random.RandomState(n).randint(0, U, n).astype(np.int32)
    _check_scores(tab, layers, users, I, guard=True)


@pytest.mark.parametrize("layers,d", WIDTH_CASES + [([10], 5), ([7, 5, 3], 3), ([128, 64], 64)])
def test_scores_on_every_width_case(layers, d):
    """one layer (no MFMA layer), widths that are no multiple of the tile, the widest stack (weights read through the
    caches instead of LDS), no GMF branch; forward(users, items) gives the same entries"""
    U, I = 11, 45
    tab = P.init_tables(U, I, d, layers, seed=sum(layers) + d)
    users = np.asarray([0, 10, 3, 3, 7], np.int32)
    eng, got = _check_scores(tab, layers, users, I)
    rs = np.random.RandomState(1)
    pu, pi = rs.randint(0, len(users), 50), rs.randint(0, I, 50).astype(np.int32)
    pairs = eng.forward(users[pu], pi).cpu().numpy()
    want = P.forward(tab, users[pu], pi, layers)[0]
    bound = 1e-5 * np.abs(want).max()
    assert np.abs(pairs - want).max() <= bound and np.abs(pairs - got[pu, pi]).max() <= bound


# ------------------------------------------------------------------ determinism, empty work, bad ids
def test_reruns_are_bit_identical(golden):
    g = golden
    runs = []
    for _ in range(2):
        eng, _ = _case_engine(g, "odd")
        loss2, losses = _loss2(eng), []
        for users, items, labels in case_feeds(g, "odd"):
            eng.step(users, items, labels, loss2)
            losses.append(loss2.cpu().numpy().copy())
        users = g["predict_users"]
        a, b = eng.score(users).cpu().numpy(), eng.score(users).cpu().numpy()
        assert np.array_equal(a, b)
        runs.append((_tables(eng), np.stack(losses), a))
    assert all(np.array_equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0])
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


def test_an_empty_batch_is_a_no_op():
    import torch
    U, I, layers, d = 9, 11, [8, 4], 3
    tab = P.init_tables(U, I, d, layers, seed=1)
    eng = _engine(tab, layers, 8)
    loss2 = torch.ones(2, device=eng.T["mlp_embedding_user"].device)
    eng.step(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), loss2)
    assert eng.t == 0 and not loss2.any().item()
    assert all(np.array_equal(v, tab[k]) for k, v in _tables(eng).items())
    assert tuple(eng.score(np.zeros(0, np.int32)).shape) == (0, I) and eng.forward([], []).numel() == 0
    _clean(eng)


def test_ids_outside_the_tables_are_refused_on_the_host():
    U, I, layers, d = 9, 11, [8, 4], 3
    eng = _engine(P.init_tables(U, I, d, layers, seed=1), layers, 8)
    loss2 = _loss2(eng)
    with pytest.raises(ValueError, match=r"NeuMF: users holds an id outside \[0, 9\)"):
        eng.step([0, 9], [1, 2], [1.0, 0.0], loss2)
    with pytest.raises(ValueError, match=r"NeuMF: items holds an id outside \[0, 11\)"):
        eng.step([0, 1], [1, -1], [1.0, 0.0], loss2)
    with pytest.raises(ValueError, match=r"users holds an id outside"):
        eng.score([9])
    with pytest.raises(ValueError, match=r"items holds an id outside"):
        eng.forward([0], [11])
    with pytest.raises(ValueError, match="batch larger than max_batch"):
        eng.step(np.zeros(9, np.int32), np.zeros(9, np.int32), np.zeros(9, np.float32), loss2)
    with pytest.raises(ValueError, match="same length"):
        eng.step([0, 1], [1, 2], [1.0], loss2)
    assert eng.t == 0


# ------------------------------------------------------------------ the drop-in runs
def _log_text(tmp_path, name):
    folder = os.path.join(str(tmp_path), "log", "ml-100k", name)
    files = os.listdir(folder)
    assert len(files) == 1
    with open(os.path.join(folder, files[0])) as f:
        return f.read()


def _check_run(tmp_path, model, name):
    text = _log_text(tmp_path, name)
    assert "%s's hyperparameters:" % name in text
    assert re.search(r"\[iter 1 : loss : [0-9.]+, time: [0-9.]+\]", text)
    shown = np.asarray([float(x) for x in re.findall(r"epoch 1:\t(.+)", text)[0].split()])
    assert np.all(np.isfinite(shown)) and shown.max() > 0
    full = model.predict([0, 5, 9], None)
    assert tuple(full.shape) == (3, model.num_items) and full.is_cuda
    full = full.cpu().numpy()
    assert np.isfinite(full).all()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1]
    bound = 1e-5 * np.abs(full).max()
    assert np.abs(cand[0] - full[0][[1, 2, 3]]).max() <= bound and np.abs(cand[1] - full[1][[7]]).max() <= bound
    return text


def test_neumf_config_drops_in(tmp_path):
    """NeuRec.properties + conf/NeuMF.properties (the reference's values) on ml-100k: one epoch through neurec_amd.main;
    the reference's log lines and a finite metric row; predict()'s modes"""
    model = _run(tmp_path, ["--recommender=NeuMF", "--epochs=1"])
    eng = model.engine
    assert (eng.d, eng.layers, eng.max_batch, eng.loss, eng.learner, eng.reg_mf, eng.reg_mlp) == \
        (16, [64, 32, 16], 256, "cross_entropy", "adam", 0.0, 0.0)
    nnz = model.dataset.train_matrix.nnz
    assert eng.t == -(-5 * nnz // 256)
    text = _check_run(tmp_path, model, "NeuMF")
    assert "load pretrained params unsuccessful!" in text


def test_mlp_config_drops_in(tmp_path):
    """conf/MLP.properties ships is_pairwise=True, which is refused by name; with the pointwise keys one epoch runs"""
    with pytest.raises(NotImplementedError, match="MLP: is_pairwise=True is not supported"):
        _run(tmp_path / "refused", ["--recommender=MLP", "--epochs=1"])
    model = _run(tmp_path, ["--recommender=MLP", "--epochs=1", "--is_pairwise=False", "--loss_function=cross_entropy"])
    eng = model.engine
    assert (eng.d, eng.layers, eng.name, eng.rows) == (0, [64, 32, 16], "MLP", ["mlp_embedding_user", "mlp_embedding_item"])
    _check_run(tmp_path, model, "MLP")
