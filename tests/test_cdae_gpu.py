"""CDAE on the GPU (csrc/cdae.hip through neurec_amd/cdae.py): every step of the reference class's trace, its recorded
epoch and predict() in both modes (tests/golden/tfgraph_cdae.npz); the batch builder against its CPU restatement
(exact); the step's gradients and whole steps on the edge shapes against the float64 restatement, which
test_cdae_cpu.py holds to the same trace; the drawn masks, determinism, empty and degenerate work, the scorer in both
modes and the drop-in run through neurec_amd.main.

The tolerance is the project's rule (`_close` of test_gru4rec_gpu.py): 4 x the float32 reference's own distance from
the float64 one for that tensor, plus 1e-5 max|want|.  For the trace the distance is the reference's, read from the
golden; for the edge shapes, which the trace does not hold, it is the restatement's float32 run."""
import os
import re

import numpy as np
import pytest

import cdae_restatement as R
from test_cdae_cpu import case_init, case_steps, epoch_steps, golden_table
from test_gru4rec_gpu import _close, _run

pytestmark = pytest.mark.gpu

BUILDER_SIZES = [1, 2, 63, 64, 65, 200]                   # around the wavefront's 64 lanes; 200 of 300 items


def _engine(tab, M, max_batch, reg=0.02, dropout=0.5, num_neg=3, act="sigmoid", loss="sigmoid_cross_entropy",
            learner="adam", seed=11, lr=0.001):
    from neurec_amd.cdae import CDAEEngine
    return CDAEEngine(tab, M, lr, reg, dropout, num_neg, max_batch, hidden_act=act, loss_func=loss, learner=learner,
                      seed=seed)


def _loss2(eng):
    import torch
    return torch.zeros(2, device=eng.T["en_offset"].device)


def _clean(eng):
    for name, G in eng.G.items():
        assert not G.any().item(), name
    for name, flag in eng.flag.items():
        assert flag is None or not flag.any().item(), name


def _same_batch(got, want):
    for k in ("entry_ptr", "items", "labels", "slot", "in_items", "in_pos"):
        assert np.array_equal(got[k].astype(np.float64), want[k].astype(np.float64)), k


def _check_batch_properties(h, indptr, indices, users, n_items):
    ptr = h["entry_ptr"]
    for s, u in enumerate(users):
        row = indices[indptr[u]:indptr[u + 1]]
        lo, hi = ptr[s], ptr[s + 1]
        neg = h["items"][lo + len(row):hi]
        assert np.array_equal(h["items"][lo:lo + len(row)], row)
        assert (np.diff(neg) > 0).all() and not np.intersect1d(neg, row).size
        assert neg.size == 0 or (neg.min() >= 0 and neg.max() < n_items)
        assert np.array_equal(h["in_items"][lo:hi], np.sort(np.concatenate([row, neg])))
        assert (h["slot"][lo:hi] == s).all()
        assert np.array_equal(h["labels"][lo:hi], np.r_[np.ones(len(row)), np.zeros(len(neg))])
    assert np.array_equal(h["in_items"][h["in_pos"]], h["items"])


# ------------------------------------------------------------------ the reference's trace
@pytest.fixture(scope="module")
def golden():
    from conftest import load_golden
    return load_golden("tfgraph_cdae")


def _case_engine(g, case, hyper_case, batch):
    import scipy.sparse as sp
    act, loss, reg, dropout, d = R.CASES[hyper_case]
    M = sp.csr_matrix((np.ones(len(g["indices"]), np.float32), g["indices"], g["indptr"]),
                      shape=tuple(int(x) for x in g["shape"]))
    init = case_init(g, case)
    return _engine(init, M, batch, reg=reg, dropout=dropout, num_neg=int(g["num_neg"]), act=act, loss=loss,
                   lr=float(g["lr"])), init, dropout


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Every variable after every step, and each step's loss, with the recorded negatives and masks handed in, against
    the f64 trace: within 4x the reference's own f32-to-f64 distance of that step and tensor (read from the golden) plus
    1e-5 max|want|.  Then predict() in both modes.  The gradient buffers and the row flags are zero again after each
    step."""
    g = golden
    eng, init, dropout = _case_engine(g, case, case, int(g["batch_step"]))
    loss2 = _loss2(eng)
    for s, (users, negs, unif) in enumerate(case_steps(g, case)):
        eng.step(users, loss2, keep=R.keep_of(unif, dropout), negatives=negs)
        l64, l32 = float(g[case + "_loss_f64"][s]), float(g[case + "_loss_f32"][s])
        _close(np.asarray([loss2.sum().item()]), np.asarray([l64]), abs(l32 - l64), "%s step %d loss" % (case, s + 1))
        for name, got in eng.tables().items():
            _close(got, golden_table(g, case, name, s, init), float(g["%s_gap_%s" % (case, name)][s]),
                   "%s step %d %s" % (case, s + 1, name))
        _clean(eng)
    assert eng.t == int(g["steps"])
    users, cand = g["predict_users"], g["predict_cand"]
    keep = R.keep_of(g["predict_%s_unif" % case], dropout)
    f32, f64 = g["predict_%s_f32" % case], g["predict_%s_f64" % case]
    got = eng.score(users, keep=keep)
    assert got.is_cuda and tuple(got.shape) == (27, 131)
    _close(got.cpu().numpy(), f64, np.abs(f32 - f64).max(), "predict %s" % case)
    got_c = eng.forward(users, cand.reshape(-1), [3] * 27, keep=keep).cpu().numpy().reshape(27, 3)
    rows = np.arange(27)[:, None]
    _close(got_c, f64[rows, cand], np.abs(f32 - f64)[rows, cand].max(), "predict %s, candidates" % case)


def test_the_recorded_epoch_ends_at_the_reference_tables(golden):
    """train_model()'s epoch of the golden, batch by batch as the class fed it (its own negatives, the session's
    uniforms), the last batch at its true size; the end tables under the trace's rule"""
    import torch
    g = golden
    eng, init, dropout = _case_engine(g, "epoch", R.EPOCH_CASE, int(g["batch_epoch"]))
    n = int(g["epoch_steps"])
    losses = torch.zeros((n, 2), device=eng.T["en_offset"].device)
    for s, (users, negs, unif) in enumerate(epoch_steps(g)):
        eng.step(users, losses[s], keep=R.keep_of(unif, dropout), negatives=negs)
    assert eng.t == n and np.isfinite(losses.cpu().numpy()).all()
    for name, got in eng.tables().items():
        _close(got, golden_table(g, "epoch", name, 0, init), float(g["epoch_gap_" + name][0]), "epoch end %s" % name)


@pytest.mark.parametrize("num_neg", [1, 5])
def test_the_batch_builder_equals_its_restatement(num_neg):
    """users of 1, 2, 63, 64, 65 and 200 items of 300 (1,000 draws from at most 100 candidates at num_neg 5), one of
    them twice in the batch: every array exactly the restatement's"""
    I = 300
    indptr, indices, M = R.csr_of(R.random_rows(BUILDER_SIZES, I, 5), I)
    eng = _engine(R.init_tables(len(BUILDER_SIZES), I, 4, 1), M, 8, num_neg=num_neg)
    users = np.asarray([5, 0, 1, 2, 3, 4, 5, 2], np.int32)
    seed = 12345 + num_neg
    batch = eng.batch(users, seed)
    h = batch.host()
    negs = R.negatives(seed, users, indptr, indices, I, num_neg)
    _same_batch(h, R.build_batch(indptr, indices, users, negs))
    _check_batch_properties(h, indptr, indices, users, I)
    assert all(np.array_equal(a, b) for a, b in zip(batch.negatives(), negs))
    assert np.array_equal(batch.negatives()[0], batch.negatives()[6])        # a draw does not depend on the slot
    if num_neg == 5:
        assert len(negs[0]) <= 100 and len(negs[0]) > 90                     # heavy de-duplication


def test_the_batch_builder_s_second_path():
    """a user whose draws exceed what a workgroup sorts in LDS sends the batch through the one sort of all keys"""
    from neurec_amd.cdae import SEGMENT_DRAWS
    I, num_neg = 4000, 5
    sizes = [3, SEGMENT_DRAWS // num_neg + 24, 65]
    assert sizes[1] * num_neg > SEGMENT_DRAWS and sizes[1] < I
    indptr, indices, M = R.csr_of(R.random_rows(sizes, I, 6), I)
    eng = _engine(R.init_tables(3, I, 1, 1), M, 4, num_neg=num_neg)
    users = np.asarray([0, 1, 2], np.int32)
    h = eng.batch(users, 99).host()
    _same_batch(h, R.build_batch(indptr, indices, users, R.negatives(99, users, indptr, indices, I, num_neg)))
    _check_batch_properties(h, indptr, indices, users, I)


def test_a_user_who_holds_every_item_has_no_negatives():
    I = 7
    indptr, indices, M = R.csr_of([np.arange(I), [2, 4]], I)
    eng = _engine(R.init_tables(2, I, 3, 1), M, 4, num_neg=2)
    h = eng.batch([0, 1], 3).host()
    assert h["entry_ptr"][1] == I and np.array_equal(h["items"][:I], np.arange(I))
    _check_batch_properties(h, indptr, indices, [0, 1], I)


# ------------------------------------------------------------------ gradients on the edge shapes
def _check_gradients(eng, tab, indptr, indices, users, keep, act, loss, reg, keep_prob, negatives=None):
    batch = eng.batch(users, 77) if negatives is None else eng.batch_given(users, negatives)
    h = batch.host()
    rb = R.build_batch(indptr, indices, users, batch.negatives())
    _same_batch(h, rb)
    E = len(rb["items"])
    keep = (np.random.RandomState(E).rand(E) < keep_prob).astype(np.uint8) if keep is None else keep(rb)
    loss2 = _loss2(eng)
    eng.gradients(batch, loss2, keep)
    (d64, r64), want = R.gradients(tab, rb, keep, keep_prob, reg, act, loss)
    (d32, r32), twin = R.gradients(tab, rb, keep, keep_prob, reg, act, loss, np.float32)
    got2 = loss2.cpu().numpy()
    _close(got2[:1], np.asarray([d64]), abs(float(d32) - d64), "loss term")
    _close(got2[1:], np.asarray([r64]), abs(float(r32) - r64), "regulariser term")
    for name, w in want.items():
        _close(eng.G[name].cpu().numpy(), w, np.abs(twin[name].astype(np.float64) - w).max(initial=0), name)
    assert eng.t == 0
    return rb, keep, want


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 128])
@pytest.mark.parametrize("act,loss", [("sigmoid", "sigmoid_cross_entropy"), ("identity", "square")])
def test_gradients_equal_the_restatement(d, B, act, loss):
    """every lane-group width and the widths around them; one slot and more slots than a workgroup's lane groups at
    d > 32 take (4); users of 1 to 12 items of 97, among them repeated users and shared items"""
    U, I, reg, dropout = 40, 97, 0.03, 0.4
    rows = R.random_rows(1 + np.random.RandomState(d).randint(0, 12, U), I, d + B)
    indptr, indices, M = R.csr_of(rows, I)
    tab = R.init_tables(U, I, d, seed=d * 7 + B)
    eng = _engine(tab, M, 33, reg=reg, dropout=dropout, act=act, loss=loss)
    users = np.random.RandomState(B).randint(0, U, B).astype(np.int32)
    if B > 1:
        users[-1] = users[0]                                                  # a repeated user
    _check_gradients(eng, tab, indptr, indices, users, None, act, loss, reg, eng.keep_prob)


@pytest.mark.parametrize("case", ["one item", "all dropped", "no dropout", "shared item"])
def test_gradients_on_degenerate_batches(case):
    U, I, d, reg = 6, 23, 20, 0.05
    rows = [[4]] + R.random_rows([3, 5, 2, 7, 4], I, 3)
    if case == "shared item":
        rows = [np.unique(np.r_[r, 11]) for r in rows]
    indptr, indices, M = R.csr_of(rows, I)
    tab = R.init_tables(U, I, d, seed=5)
    dropout = 0.0 if case == "no dropout" else 0.5
    eng = _engine(tab, M, 8, reg=reg, dropout=dropout, loss="square")
    users = np.asarray([0] if case == "one item" else [0, 1, 2, 3, 4, 5], np.int32)

    def keep(rb):
        k = (np.random.RandomState(1).rand(len(rb["items"])) < 0.5).astype(np.uint8)
        if case == "no dropout":
            k[:] = 1
        if case == "all dropped":
            k[rb["entry_ptr"][-2]:rb["entry_ptr"][-1]] = 0                    # the last slot's whole input row
        return k
    rb, k, want = _check_gradients(eng, tab, indptr, indices, users, keep, "sigmoid", "square", reg, eng.keep_prob)
    if case == "all dropped":
        lo = rb["entry_ptr"][-2]
        assert len(k) - lo >= 5 and not k[lo:].any() and k[:lo].any()
        z = tab["user_embeddings"][5].astype(np.float64) + tab["en_offset"]        # the slot's hidden: its own row
        assert np.abs(eng._hidden[5].cpu().numpy() - 1.0 / (1.0 + np.exp(-z))).max() <= 1e-6
    if case == "shared item":
        assert all(11 in rb["items"][rb["entry_ptr"][s]:rb["entry_ptr"][s + 1]] for s in range(len(users)))


def test_the_learners_flags_mark_the_batch_s_rows():
    U, I, d = 6, 23, 5
    indptr, indices, M = R.csr_of(R.random_rows([3, 5, 2, 7, 4, 1], I, 3), I)
    eng = _engine(R.init_tables(U, I, d, 2), M, 8, learner="gd")
    batch = eng.batch([1, 4, 1], 5)
    eng.gradients(batch, _loss2(eng))
    items = np.unique(batch.host()["items"])
    for name in ("de_embeddings", "de_bias"):                  # en_embeddings takes the dense application: no flags
        assert np.array_equal(np.flatnonzero(eng.flag[name].cpu().numpy()), items), name
    assert sorted(eng.flag) == ["de_bias", "de_embeddings", "user_embeddings"]
    assert np.array_equal(np.flatnonzero(eng.flag["user_embeddings"].cpu().numpy()), [1, 4])
    eng.apply()
    _clean(eng)


# ------------------------------------------------------------------ whole steps
@pytest.mark.parametrize("act,loss,reg,dropout,d", [("sigmoid", "sigmoid_cross_entropy", 0.01, 0.5, 9),
                                                   ("identity", "square", 0.0, 0.0, 16),
                                                   ("sigmoid", "square", 0.02, 0.5, 33),
                                                   ("identity", "sigmoid_cross_entropy", 0.0, 0.5, 7)])
def test_steps_follow_the_restatement(act, loss, reg, dropout, d):
    """four steps of Adam with the device's own negatives and given masks: every variable after every step and each
    loss against the float64 restatement, the float32 restatement's distance as the bar; gradient buffers and flags
    zero again after each step"""
    U, I, lr = 30, 61, 0.01
    rows = R.random_rows(1 + np.random.RandomState(d).randint(0, 9, U), I, d)
    indptr, indices, M = R.csr_of(rows, I)
    tab = R.init_tables(U, I, d, seed=d)
    eng = _engine(tab, M, 12, reg=reg, dropout=dropout, act=act, loss=loss, lr=lr, seed=4)
    a64, a32 = R.Adam(tab, lr), R.Adam(tab, lr, np.float32)
    loss2 = _loss2(eng)
    rs = np.random.RandomState(8)
    for s in range(4):
        users = rs.randint(0, U, 12).astype(np.int32)
        users[5] = users[2]
        negs = R.negatives(R.step_seed(4, s), users, indptr, indices, I, 3)
        rb = R.build_batch(indptr, indices, users, negs)
        keep = (rs.rand(len(rb["items"])) < eng.keep_prob).astype(np.uint8)
        eng.step(users, loss2, keep)
        (l64, r64), G64 = R.gradients(a64.T, rb, keep, eng.keep_prob, reg, act, loss)
        (l32, r32), G32 = R.gradients(a32.T, rb, keep, eng.keep_prob, reg, act, loss, np.float32)
        a64.apply(G64)
        a32.apply(G32)
        _close(np.asarray([loss2.sum().item()]), np.asarray([l64 + r64]), abs(float(l32) + float(r32) - l64 - r64),
               "step %d loss" % (s + 1))
        for name, got in eng.tables().items():
            _close(got, a64.T[name], np.abs(a32.T[name].astype(np.float64) - a64.T[name]).max(),
                   "step %d %s" % (s + 1, name))
        _clean(eng)
    assert eng.t == 4


def test_reruns_are_bit_identical():
    U, I, d = 30, 61, 24
    indptr, indices, M = R.csr_of(R.random_rows(1 + np.random.RandomState(1).randint(0, 9, U), I, 2), I)
    tab = R.init_tables(U, I, d, seed=3)
    runs = []
    for _ in range(2):
        eng = _engine(tab, M, 16, seed=21)
        loss2, losses = _loss2(eng), []
        rs = np.random.RandomState(5)
        for s in range(3):
            eng.step(rs.randint(0, U, 16).astype(np.int32), loss2)            # negatives and masks drawn
            losses.append(loss2.cpu().numpy().copy())
        runs.append((eng.tables(), np.stack(losses), eng.score(np.arange(U)).cpu().numpy()))
    assert all(np.array_equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0])
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    assert not all(np.array_equal(runs[0][0][k], tab[k]) for k in tab)


# ------------------------------------------------------------------ drawn masks
def test_drawn_masks_are_the_restated_generator_s():
    """the step writes the mask it drew; the encoder of predict() too.  Over 20,000 entries at keep 0.5 the kept share
    lies within five binomial standard deviations (0.018) of 0.5 (checked for this seed on the CPU as well)"""
    U, I, d = 100, 1000, 3
    indptr, indices, M = R.csr_of(R.random_rows([200] * U, I, 9), I)
    eng = _engine(R.init_tables(U, I, d, 1), M, 8, dropout=0.5, seed=2018)
    batch = eng.batch([3, 7, 3], 1)
    eng.gradients(batch, _loss2(eng))
    E = int(batch.host()["entry_ptr"][-1])
    assert np.array_equal(eng.last_keep[:E].cpu().numpy(), R.mask(2018, 0, E, eng.keep_prob))
    eng.hidden(np.arange(U))
    got = eng.last_keep[:20000].cpu().numpy()
    assert np.array_equal(got, R.mask(2018 + 1, 1, 20000, eng.keep_prob))
    assert abs(got.mean() - 0.5) <= 0.018, got.mean()
    eng.hidden(np.arange(U))
    assert not np.array_equal(eng.last_keep[:20000].cpu().numpy(), got)       # a fresh mask per call


# ------------------------------------------------------------------ empty and degenerate work, the scorer
def test_an_empty_batch_is_a_no_op():
    import torch
    U, I, d = 5, 11, 4
    indptr, indices, M = R.csr_of(R.random_rows([3, 0, 2, 1, 4], I, 1), I)
    tab = R.init_tables(U, I, d, 1)
    eng = _engine(tab, M, 8)
    loss2 = torch.ones(2, device=eng.T["en_offset"].device)
    eng.step(np.zeros(0, np.int32), loss2)
    assert eng.t == 0 and eng.adam.t == 0 and loss2.cpu().numpy().tolist() == [1.0, 1.0]
    assert all(np.array_equal(v, tab[k]) for k, v in eng.tables().items())
    assert tuple(eng.score(np.zeros(0, np.int32)).shape) == (0, I) and eng.forward([], []).numel() == 0
    assert eng.batch([], 1).B == 0
    _clean(eng)
    with pytest.raises(ValueError, match=r"user ids must lie in \[0, 5\)"):
        eng.step([5], loss2)
    with pytest.raises(ValueError, match="batch larger than max_batch"):
        eng.step(np.zeros(9, np.int32), loss2)


@pytest.mark.parametrize("act", ["sigmoid", "identity"])
def test_a_user_without_train_items_scores_its_own_row(act):
    U, I, d = 5, 11, 4
    indptr, indices, M = R.csr_of(R.random_rows([3, 0, 2, 1, 4], I, 1), I)
    tab = R.init_tables(U, I, d, 2)
    eng = _engine(tab, M, 8, act=act)
    z = tab["user_embeddings"][1].astype(np.float64) + tab["en_offset"]
    h = z if act == "identity" else 1.0 / (1.0 + np.exp(-z))
    want = h @ tab["de_embeddings"].astype(np.float64).T + tab["de_bias"]
    got = eng.score([1]).cpu().numpy()[0]
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


def test_the_scorer_s_two_modes_agree_and_match_the_restatement():
    """27 users x 131 items: score() is a device tensor [27, 131]; forward() on every pair gives the same entries;
    with a given mask both follow predict() of the restatement"""
    U, I, d = 40, 131, 19
    indptr, indices, M = R.csr_of(R.random_rows(np.random.RandomState(2).randint(0, 15, U), I, 4), I)
    tab = R.init_tables(U, I, d, 3)
    eng = _engine(tab, M, 8)
    users = np.sort(np.random.RandomState(3).choice(U, 27, replace=False)).astype(np.int32)
    full = eng.score(users, keep_prob=1.0)
    assert full.is_cuda and tuple(full.shape) == (27, 131)
    full = full.cpu().numpy()
    pairs = eng.forward(users, np.tile(np.arange(I, dtype=np.int32), 27), [I] * 27, keep_prob=1.0).cpu().numpy()
    bound = 1e-5 * np.abs(full).max()
    assert np.abs(pairs.reshape(27, I) - full).max() <= bound
    n = int(sum(indptr[u + 1] - indptr[u] for u in users))
    want, _ = R.predict(tab, indptr, indices, users, np.ones(n), 1.0, "sigmoid")
    assert np.abs(full - want).max() <= 1e-5 * np.abs(want).max()
    keep = (np.random.RandomState(4).rand(n) < 0.5).astype(np.uint8)
    want, hid = R.predict(tab, indptr, indices, users, keep, eng.keep_prob, "sigmoid")
    got = eng.score(users, keep=keep).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert np.abs(eng.hidden(users, keep=keep).cpu().numpy() - hid).max() <= 1e-5 * np.abs(hid).max()
    cand = eng.forward(users[:2], [5, 6, 130], [2, 1], keep=keep).cpu().numpy()
    assert np.abs(cand - want[[0, 0, 1], [5, 6, 130]]).max() <= bound


# ------------------------------------------------------------------ the drop-in run
def _recall10(header, row):
    names = [x.strip() for x in header.split("\t")[1:]]
    return float(row.split()[names.index("Recall@10")])


def test_cdae_config_drops_in(tmp_path):
    """NeuRec.properties + conf/CDAE.properties on ml-100k through neurec_amd.main, two epochs at hidden_dim 8: the
    reference's log lines, finite losses, and Recall@10 after epoch 1 above the untrained tables' on the same split (a
    sanity check, not a quality claim)"""
    argv = ["--recommender=CDAE", "--hidden_dim=8", "--lr=0.01"]
    fresh = _run(tmp_path / "fresh", argv + ["--epochs=0"])
    header = fresh.evaluator.metrics_info()
    before = _recall10(header, fresh.evaluate_model())
    model = _run(tmp_path / "run", argv + ["--epochs=2"])
    eng = model.engine
    assert (eng.d, eng.num_neg, eng.max_batch, eng.hidden_act, eng.loss_func, eng.learner) == \
        (8, 5, 32, "sigmoid", "sigmoid_cross_entropy", "adam")
    assert abs(eng.keep_prob - 0.5) < 1e-7 and abs(eng.reg - 0.001) < 1e-12
    n_users = int((np.diff(model.train_csr_mat.indptr) > 0).sum())
    assert eng.t == 2 * -(-n_users // 32)
    folder = os.path.join(str(tmp_path / "run"), "log", "ml-100k", "CDAE")
    files = os.listdir(folder)
    assert len(files) == 1
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "CDAE's hyperparameters:" in text and "metrics:\t" in text
    shown = re.findall(r"epoch (\d+):\t(.+)", text)
    assert [int(n) for n, _ in shown] == [0, 1]
    assert np.isfinite(model.losses.cpu().numpy()).all() and model.losses.cpu().numpy()[:, 0].min() > 0
    after = _recall10(header, shown[1][1])
    print("Recall@10 untrained %.4f, after two epochs %.4f" % (before, after))
    assert after > before
    full = model.predict([0, 5, 9], None)
    assert full.is_cuda and tuple(full.shape) == (3, model.num_items) and np.isfinite(full.cpu().numpy()).all()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and all(isinstance(c, np.ndarray) for c in cand)
