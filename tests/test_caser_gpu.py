"""Caser on the GPU (csrc/caser.hip through neurec_amd/caser.py): every step of the reference class's trace, the recorded
epoch through run_schedule, predict(), the edge shapes of the step on its gradients, saturated logits, determinism,
empty work, ids outside the tables, the refusals and the drop-in run through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import caser_restatement as P
from caser_restatement import CASES
from test_caser_cpu import case_init, case_inputs, golden_table
from test_gru4rec_gpu import _close, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_caser")


def _engine(tab, T, N, nv, nh, max_batch, lr=0.001, l2=0.0, rate=0.0, seed=2017):
    from neurec_amd.caser import CaserEngine
    return CaserEngine(tab, lr, l2, max_batch, T, N, nv, nh, rate, seed=seed)


def _dev(eng, a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(eng.item_embeddings.device)


def _tables(eng):
    return {k: t.cpu().numpy() for k, t in eng.tables().items()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Every variable after every step, and each step's loss, against the f64 trace: within 4x the reference's own
    f32-to-f64 distance of that step and tensor (read from the golden) plus 1e-5 max|want|.  The gradient buffers are
    zero again afterwards."""
    import torch
    g = golden
    d, L, T, N, nv, nh, l2, rate = CASES[case]
    names, init, feeds, masks = case_inputs(g, case)
    eng = _engine(init, T, N, nv, nh, int(g["batch_step"]), float(g["lr"]), l2, rate)
    assert list(eng.tables()) == names
    loss2 = torch.zeros(2, device=eng.item_embeddings.device)
    for s, (users, seq, pos, neg) in enumerate(feeds):
        eng.step(users, seq, pos, neg, loss2, None if masks is None else _dev(eng, masks[s], np.uint8))
        l64, l32 = float(g[case + "_loss_f64"][s]), float(g[case + "_loss_f32"][s])
        _close(np.asarray([loss2.sum().item()]), np.asarray([l64]), abs(l32 - l64), "%s step %d loss" % (case, s + 1))
        for name, got in _tables(eng).items():
            _close(got, golden_table(g, case, name, s, init), float(g["%s_gap_%s" % (case, name)][s]),
                   "%s step %d %s" % (case, s + 1, name))
    assert eng.t == len(feeds)
    for name, G in eng.G.items():
        assert not G.any().item(), name


def test_the_recorded_epoch_ends_at_the_reference_tables(golden):
    """train_model()'s epoch of the golden (rate 0, pad targets among its positives) through run_schedule, the last
    batch cut to its true size; the end tables under the trace's rule"""
    import torch
    g = golden
    d, L, T, N, nv, nh, l2, _ = CASES["first"]
    init = case_init(g, "epoch")
    eng = _engine(init, T, N, nv, nh, int(g["batch_epoch"]), float(g["lr"]), l2, 0.0)
    S = len(g["epoch_seq"])
    losses = torch.zeros((S, 2), device=eng.item_embeddings.device)
    eng.run_schedule(g["epoch_users"], g["epoch_seq"], g["epoch_pos"], g["epoch_neg"], losses, g["epoch_rows"])
    assert eng.t == S and np.isfinite(losses.cpu().numpy()).all()
    for name, got in _tables(eng).items():
        _close(got, golden_table(g, "epoch", name, 0, init), float(g["epoch_gap_" + name][0]), "epoch end %s" % name)


def test_predict_matches_the_reference(golden):
    """predict(), full and candidate mode, after the trained case, under the trace's rule: no item bias in it"""
    import torch
    g = golden
    case = P.PREDICT_CASE
    d, L, T, N, nv, nh, l2, rate = CASES[case]
    names, init, feeds, masks = case_inputs(g, case)
    eng = _engine(init, T, N, nv, nh, int(g["batch_step"]), float(g["lr"]), l2, rate)
    loss2 = torch.zeros(2, device=eng.item_embeddings.device)
    for s, (users, seq, pos, neg) in enumerate(feeds):
        eng.step(users, seq, pos, neg, loss2, _dev(eng, masks[s], np.uint8))
    eng.set_sequences(g["seq_ptr"], g["seq"])
    users, cand = g["predict_users"], g["predict_cand"]
    got = eng.score(users)
    assert got.is_cuda and tuple(got.shape) == (len(users), eng.n_items)
    got = got.cpu().numpy()
    _close(got, g["predict_f64"], np.abs(g["predict_f32"] - g["predict_f64"]).max(), "predict")
    got_c = np.stack([got[k][c] for k, c in enumerate(cand)])
    _close(got_c, g["predict_cand_f64"], np.abs(g["predict_cand_f32"] - g["predict_cand_f64"]).max(),
           "predict, candidates")
    assert np.abs(eng.T["item_biases"].cpu().numpy()).max() > 0.01
    # a user without train items scores concat(z of the all-padded row, its user row)
    eng.set_sequences(np.zeros(len(g["seq_ptr"]), np.int64), np.zeros(0, np.int32))
    tab = _tables(eng)
    row = eng.score([3]).cpu().numpy()[0]
    want = P.scores(tab, [3], np.full((1, L), eng.n_items), eng.n_items, nv, nh)[0]
    assert np.abs(row - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("d", [64, 65, 128])
def test_scores_on_both_sides_of_the_shared_kernel_s_width(d):
    """2 d <= 128 goes through nrhip_gru4rec_scores, wider rows through nrhip_caser_scores"""
    U, I, L, T, N, nv, nh = 6, 70, 3, 1, 1, 2, 2
    tab = P.init_tables(U, I, d, L, nv, nh, seed=d)
    eng = _engine(tab, T, N, nv, nh, 4)
    users = np.arange(U, dtype=np.int32)
    seq = np.random.RandomState(d).randint(0, I + 1, (U, L)).astype(np.int32)
    got = eng.score_rows(users, seq).cpu().numpy()                   # six rows through max_batch 4: two forward calls
    want = P.scores(tab, users, seq, I, nv, nh)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


# ------------------------------------------------------------------ edges of the step
def _batch(U, I, L, T, N, B, seed, pads=None):
    """B rows; pads[b] front pads of row b's sequence (drawn when None)"""
    rs = np.random.RandomState(seed)
    users = rs.randint(0, U, B).astype(np.int32)
    seq = rs.randint(0, I, (B, L)).astype(np.int32)
    pads = rs.randint(0, L + 1, B).tolist() if pads is None else pads
    for b in range(B):
        seq[b, :min(pads[b], L)] = I
    return users, seq, rs.randint(0, I, (B, T)).astype(np.int32), rs.randint(0, I, (B, N)).astype(np.int32)


def _check_gradients(tab, users, seq, pos, neg, I, nv, nh, rate=0.0, l2=0.0, mask=None):
    """gradients() against the float64 restatement with TF's even split: 1e-5 max|want| per tensor (fp32 sums of at most
    a few thousand terms of the tensor's own size, each carrying a few 2^-24).  Adam is left out on purpose: its first
    step is lr sign(g) and hides the size of an error (test_sasrec_gpu._check_gradients)."""
    import torch
    B, T, N = len(users), pos.shape[1], neg.shape[1]
    eng = _engine(tab, T, N, nv, nh, B, 0.001, l2, rate)
    before = _tables(eng)
    loss2 = torch.zeros(2, device=eng.item_embeddings.device)
    eng.gradients(users, seq, pos, neg, loss2, None if mask is None else _dev(eng, mask, np.uint8))
    want_loss, G = P.gradients(tab, users, seq, pos, neg, I, nv, nh, rate, l2, mask, "even")
    got_loss = float(loss2.cpu().numpy().astype(np.float64).sum())
    print("loss: got %.9g want %.9g" % (got_loss, want_loss))
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss)
    for name, want in G.items():
        got = eng.G[name].cpu().numpy()
        err = np.abs(got - want).max()
        print("%s: err %.3g, max|want| %.3g" % (name, err, np.abs(want).max()))
        assert np.isfinite(got).all() and err <= 1e-5 * np.abs(want).max(), (name, err)
    for name, t in _tables(eng).items():                           # gradients() moves no table
        assert np.array_equal(t, before[name]), name
    return eng


@pytest.mark.parametrize("d,L,T,N,nv,nh,B", [
    (6, 4, 2, 3, 2, 3, 1),                # B = 1
    (5, 3, 2, 2, 2, 3, 257),              # B = 257: more rows than the chunks of the variable gradients hold singly
    (6, 1, 1, 2, 2, 3, 5),                # L = 1
    (128, 10, 3, 3, 2, 3, 3),             # the longest window at the widest row
    (1, 4, 2, 2, 3, 2, 5),                # d = 1
    (6, 4, 16, 16, 16, 64, 4),            # the most filters and the most targets
    (50, 5, 3, 3, 4, 16, 9),              # the defaults' odd width
])
def test_gradients_at_the_edge_shapes(d, L, T, N, nv, nh, B):
    U, I = 11, 23
    tab = P.init_tables(U, I, d, L, nv, nh, seed=d + L)
    users, seq, pos, neg = _batch(U, I, L, T, N, B, seed=B)
    _check_gradients(tab, users, seq, pos, neg, I, nv, nh, l2=0.01)


def test_gradients_of_awkward_rows():
    """an all-pad row, one user in every row, a repeated item under height 1, a pad target, the same item as positive
    and negative, and a mask that drops every feature of a row"""
    U, I, d, L, T, N, nv, nh, B = 7, 23, 6, 4, 2, 2, 3, 4, 6
    tab = P.init_tables(U, I, d, L, nv, nh, seed=5)
    users, seq, pos, neg = _batch(U, I, L, T, N, B, seed=2, pads=[4, 0, 3, 1, 0, 2])
    users[:] = 4
    seq[1] = 5
    pos[0, 0] = I
    neg[2, 0] = pos[2, 1]
    rs = np.random.RandomState(1)
    mask = (rs.rand(B, nv * d + nh * L) < 0.6).astype(np.uint8)
    mask[3] = 0
    eng = _check_gradients(tab, users, seq, pos, neg, I, nv, nh, rate=0.4, mask=mask)
    G = {k: v.cpu().numpy() for k, v in eng.G.items()}
    assert np.flatnonzero(np.abs(G["user_embeddings"]).max(axis=1)).tolist() == [4]
    # without a regulariser the rows outside the batch are untouched
    outside = np.setdiff1d(np.arange(I), seq.reshape(-1))
    assert len(outside) and not G["seq_item_embeddings"][outside].any()
    outside = np.setdiff1d(np.arange(I), np.concatenate([pos.reshape(-1), neg.reshape(-1)]))
    assert len(outside) and not G["item_embeddings"][outside].any() and not G["item_biases"][outside].any()
    # the all-ones mask at rate 0.5 doubles the features: the scale 1 / (1 - rate) is there
    _check_gradients(tab, users, seq, pos, neg, I, nv, nh, rate=0.5, mask=np.ones_like(mask))


def test_saturated_logits():
    """logits set through the item biases (item_embeddings is zero), in |x| <= 8 and in |x| >= 30, none between,
    against the float32 restatement of the expression as it is written.  Where 1 - sigmoid(x) is formed, two float32
    roundings of 2^-24 each (exp, the division) sit in front of it, so a term and its derivative may differ by 2^-23 /
    (1 - sigmoid(8)) = 3.6e-4 of their size between two correct float32 evaluations; that bounds the comparison.  The
    saturated terms are exact: -log(1e-24) and gradient 0 — a softplus would give |x| and 1."""
    import torch
    U, I, d, L, T, N, nv, nh = 4, 16, 4, 3, 4, 4, 2, 2
    tab = P.init_tables(U, I, d, L, nv, nh, seed=8)
    tab["item_embeddings"] = np.zeros_like(tab["item_embeddings"])
    logit = np.asarray([-8.0, -3.0, -1.0, 0.0, 0.5, 2.0, 4.0, 8.0, 30.0, 50.0, 100.0, -30.0, -50.0, -100.0, 31.0, -31.0])
    tab["item_biases"] = logit.astype(np.float32)
    users = np.asarray([0, 1, 2, 3], np.int32)
    seq = np.asarray([[1, 2, 3], [I, 4, 5], [I, I, 6], [7, 8, 9]], np.int32)
    pos = np.asarray([[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]], np.int32)
    neg = pos[::-1].copy()
    eng = _engine(tab, T, N, nv, nh, 4)
    loss2 = torch.zeros(2, device=eng.item_embeddings.device)
    eng.gradients(users, seq, pos, neg, loss2)
    want_loss, G = P.gradients(tab, users, seq, pos, neg, I, nv, nh, dtype=np.float32)
    rel = 2.0 ** -23 / (1.0 - 1.0 / (1.0 + np.exp(-8.0)))
    got = float(loss2[0].item())
    print("loss got %.7g want %.7g" % (got, want_loss))
    cap = float(-np.log(np.float32(1e-24)))
    assert want_loss > 5 * cap / 16                                 # five terms sit at the cap
    assert abs(got - float(want_loss)) <= rel * abs(float(want_loss))
    gb = eng.G["item_biases"].cpu().numpy()
    assert np.abs(gb - G["item_biases"]).max() <= rel * np.abs(G["item_biases"]).max()
    # every target saturated: positives at +30 and beyond cost -log(1 + 1e-24) = 0, negatives there exactly
    # -log(1e-24); every gradient is exactly zero
    big = np.asarray([[8, 9, 10, 14]] * 4, np.int32)
    for G2 in eng.G.values():                                       # gradients() asks for zero buffers
        G2.zero_()
    eng.gradients(users, seq, big, big, loss2)
    assert abs(float(loss2[0].item()) - cap) <= 1e-6 * cap
    for name, G2 in eng.G.items():
        assert not G2.any().item(), name
    # ... and positives at -100: sigmoid is 0 in float32
    low = np.asarray([[13, 13, 13, 13]] * 4, np.int32)
    eng.gradients(users, seq, low, big, loss2)
    assert abs(float(loss2[0].item()) - 2 * cap) <= 1e-6 * 2 * cap
    for name, G2 in eng.G.items():
        assert not G2.any().item(), name


def test_two_runs_are_bit_identical_and_the_buffers_end_zero():
    import torch
    U, I, d, L, T, N, nv, nh, B = 30, 40, 50, 5, 3, 3, 4, 16, 33
    tab = P.init_tables(U, I, d, L, nv, nh, seed=4)
    users, seq, pos, neg = _batch(U, I, L, T, N, B, seed=9)
    runs = []
    for _ in range(2):
        eng = _engine(tab, T, N, nv, nh, B, rate=0.5, l2=0.01, seed=77)
        loss2 = torch.zeros(2, device=eng.item_embeddings.device)
        eng.gradients(users, seq, pos, neg, loss2)
        grads = {k: v.cpu().numpy().copy() for k, v in eng.G.items()}
        eng.apply()
        for name, G in eng.G.items():
            assert not G.any().item(), name
        eng.step(users, seq, pos, neg, loss2)                       # the generator's second step differs from its first
        runs.append((grads, _tables(eng), loss2.cpu().numpy().copy()))
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k
    assert np.array_equal(runs[0][2], runs[1][2])
    # the generator drops about half of the features: the gradients differ from the rate-0 ones
    eng0 = _engine(tab, T, N, nv, nh, B, rate=0.0, l2=0.01)
    eng0.gradients(users, seq, pos, neg, loss2)
    assert not np.array_equal(eng0.G["fc1_kernel"].cpu().numpy(), runs[0][0]["fc1_kernel"])


def test_an_empty_batch_is_no_work():
    import torch
    U, I, d, L, T, N, nv, nh = 5, 9, 6, 4, 2, 3, 2, 3
    eng = _engine(P.init_tables(U, I, d, L, nv, nh, seed=6), T, N, nv, nh, 4)
    before = _tables(eng)
    loss2 = torch.ones(2, device=eng.item_embeddings.device)
    eng.step(np.zeros(0, np.int32), np.zeros((0, L), np.int32), np.zeros((0, T), np.int32), np.zeros((0, N), np.int32),
             loss2)
    assert eng.t == 0 and not loss2.any().item()
    for name, t in _tables(eng).items():
        assert np.array_equal(t, before[name]), name
    for name, G in eng.G.items():
        assert not G.any().item(), name
    losses = torch.zeros((2, 2), device=eng.item_embeddings.device)
    users, seq, pos, neg = _batch(U, I, L, T, N, 3, seed=1)
    eng.run_schedule(np.stack([users, users]), np.stack([seq, seq]), np.stack([pos, pos]), np.stack([neg, neg]), losses,
                     rows=[0, 3])
    assert eng.t == 1 and not losses[0].any().item() and losses[1, 0].item() > 0
    eng.set_sequences(np.zeros(U + 1, np.int64), np.zeros(0, np.int32))
    assert tuple(eng.score([]).shape) == (0, I)


def test_ids_outside_the_tables():
    import torch
    U, I, d, L, T, N, nv, nh = 5, 9, 6, 4, 2, 3, 2, 3
    eng = _engine(P.init_tables(U, I, d, L, nv, nh, seed=6), T, N, nv, nh, 4)
    loss2 = torch.zeros(2, device=eng.item_embeddings.device)
    feeds = _batch(U, I, L, T, N, 3, seed=1)
    for k, (name, bads, text) in enumerate((("users", (-1, U), r"\[0, 5\)"), ("seq", (-1, I + 1), r"\[0, 9\]"),
                                            ("pos", (-1, I + 1), r"\[0, 9\]"), ("neg", (-1, I), r"\[0, 9\)"))):
        for bad in bads:
            arrs = [a.copy() for a in feeds]
            arrs[k].reshape(-1)[-1] = bad
            with pytest.raises(ValueError, match="%s holds an id outside %s" % (name, text)):
                eng.step(*arrs, loss2)
            with pytest.raises(ValueError, match="%s holds an id outside %s" % (name, text)):
                eng.run_schedule(*[a[None] for a in arrs], loss2[None])
    with pytest.raises(ValueError, match=r"seq holds an item outside \[0, 9\)"):
        eng.set_sequences(np.asarray([0, 2]), np.asarray([1, 9]))
    assert eng.t == 0
    # device tensors are not read back: an id outside the table reads a zero row and its gradient is dropped
    users, seq, pos, neg = feeds
    bad_seq, bad_pos = seq.copy(), pos.copy()
    bad_seq[1, -1], bad_pos[2, 0] = I + 3, -2
    eng.gradients(*[_dev(eng, a, np.int32) for a in (users, bad_seq, bad_pos, neg)], loss2)
    got = {k: v.cpu().numpy().copy() for k, v in eng.G.items()}
    for G in eng.G.values():
        G.zero_()
    as_pad_seq, as_pad_pos = seq.copy(), pos.copy()
    as_pad_seq[1, -1], as_pad_pos[2, 0] = I, I
    eng.gradients(users, as_pad_seq, as_pad_pos, neg, loss2)
    for k, v in eng.G.items():
        assert np.array_equal(v.cpu().numpy(), got[k]), k


def test_refusals_on_the_device():
    import torch
    U, I, d, L, T, N, nv, nh = 5, 9, 6, 4, 2, 3, 2, 3
    eng = _engine(P.init_tables(U, I, d, L, nv, nh, seed=6), T, N, nv, nh, 2, rate=0.5)
    loss2 = torch.zeros(2, device=eng.item_embeddings.device)
    users, seq, pos, neg = _batch(U, I, L, T, N, 3, seed=1)
    with pytest.raises(ValueError, match="batch larger than max_batch"):
        eng.gradients(users, seq, pos, neg, loss2)
    with pytest.raises(ValueError, match=r"seq \[batch, seq_L\]"):
        eng.gradients(users[:2], seq[:2, :3], pos[:2], neg[:2], loss2)
    with pytest.raises(ValueError, match=r"pos \[batch, seq_T\]"):
        eng.gradients(users[:2], seq[:2], pos[:2, :1], neg[:2], loss2)
    with pytest.raises(ValueError, match=r"mask must be \[batch, nv factors_num \+ nh seq_L\] = \(2, 24\)"):
        eng.gradients(users[:2], seq[:2], pos[:2], neg[:2], loss2, _dev(eng, np.ones((2, 23)), np.uint8))
    with pytest.raises(ValueError, match="set_sequences"):
        eng.score([0])
    assert eng.t == 0


# ------------------------------------------------------------------ the drop-in run
def test_caser_config_drops_in(tmp_path):
    """NeuRec.properties + conf/Caser.properties (the reference's values) on ml-100k with by_time=True: two epochs
    through neurec_amd.main; the metrics header, the deviation line and two `epoch` lines, in order; predict()'s modes"""
    from neurec_amd.model.sequential_recommender.Caser import DEVIATIONS
    model = _run(tmp_path, ["--recommender=Caser", "--epochs=2"])
    eng = model.engine
    assert (eng.d, eng.L, eng.seq_T, eng.neg_samples, eng.nv, eng.nh, eng.max_batch, eng.rate, eng.l2_reg) == \
        (50, 5, 3, 3, 4, 16, 256, 0.5, 0.001)
    n_rows = sum(max(1, len(items) - 8 + 1) for items in model.user_pos_train.values())
    assert eng.t == 2 * -(-n_rows // 256)
    folder = os.path.join(str(tmp_path), "log", "ml-100k", "Caser")
    files = os.listdir(folder)
    assert len(files) == 1
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "Caser's hyperparameters:" in text
    lines = [ln for ln in text.splitlines() if re.search(r"metrics:\t|epoch \d+:\t", ln) or DEVIATIONS in ln]
    kinds = ["m" if "metrics:" in ln else "d" if DEVIATIONS in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)
             for ln in lines]
    assert kinds == ["m", "d", "e0", "e1"], kinds
    shown = np.asarray([float(x) for x in re.findall(r"epoch 1:\t(.+)", text)[0].split()])
    assert np.all(np.isfinite(shown)) and shown.max() > 0
    full = model.predict([0, 5, 9], None)
    assert tuple(full.shape) == (3, model.items_num) and full.is_cuda
    full = full.cpu().numpy()
    assert np.isfinite(full).all()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])
    assert np.array_equal(cand[1], full[1][[7]])


def test_plugin_refusals(tmp_path):
    with pytest.raises(NotImplementedError, match=r"seq_L=11 is not supported \(1 to 10\)"):
        _run(tmp_path, ["--recommender=Caser", "--epochs=1", "--seq_L=11"])
    with pytest.raises(NotImplementedError, match=r"nh=65 is not supported \(1 to 64\)"):
        _run(tmp_path, ["--recommender=Caser", "--epochs=1", "--nh=65"])
