"""SRGNN on the GPU (csrc/srgnn.hip through neurec_amd/srgnn.py): every step of the reference class's trace, the recorded
epoch through run_schedule, predict(), the edge shapes of the step against the restatement, saturated logits, the guard
row, determinism, a user without items, score batching, the refusals and the drop-in run through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import srgnn_restatement as P
from test_gru4rec_gpu import _close, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_srgnn")


def _engine(tab, L, step, max_batch, lr=0.001, l2=0.0, nonhybrid=False):
    from neurec_amd.srgnn import SRGNNEngine
    return SRGNNEngine(tab, lr, l2, max_batch, L, step, nonhybrid)


def _tables(eng):
    return {k: t.cpu().numpy() for k, t in eng.tables().items()}


def _loss2(eng):
    import torch
    return torch.zeros(2, device=eng.T["embedding"].device)


# ------------------------------------------------------------------ the reference's trace
def _case(g, case):
    from test_srgnn_cpu import CASES, case_init
    d, step, nonhybrid, l2, L, _ = CASES[case]
    return d, step, nonhybrid, l2, L, case_init(g, case)


@pytest.mark.parametrize("case", ["hybrid", "gated", "repeats"])
def test_steps_match_the_reference_trace(golden, case):
    """Every variable after every step, and each step's loss, against the f64 trace: within 4x the reference's own
    f32-to-f64 distance of that step and tensor (read from the golden) plus 1e-5 max|want|.  The gradient buffers are
    zero again afterwards."""
    from test_srgnn_cpu import golden_table
    g = golden
    d, step, nonhybrid, l2, L, init = _case(g, case)
    eng = _engine(init, L, step, int(g["batch_step"]), float(g["lr"]), l2, nonhybrid)
    assert list(eng.tables()) == list(P.NAMES)
    loss2 = _loss2(eng)
    for s in range(len(g[case + "_seq"])):
        eng.step(g[case + "_seq"][s], g[case + "_target"][s], loss2, float(g[case + "_lrs"][s]))
        l64, l32 = float(g[case + "_loss_f64"][s]), float(g[case + "_loss_f32"][s])
        _close(np.asarray([loss2.sum().item()]), np.asarray([l64]), abs(l32 - l64), "%s step %d loss" % (case, s + 1))
        for name, got in _tables(eng).items():
            _close(got, golden_table(g, case, name, s, init), float(g["%s_gap_%s" % (case, name)][s]),
                   "%s step %d %s" % (case, s + 1, name))
        for name, G in eng.G.items():
            assert not G.any().item(), name
    if case == "gated":                                              # nonhybrid at L2 = 0: B stays put
        assert np.array_equal(_tables(eng)["B"], init["B"])


def test_the_recorded_epoch_ends_at_the_reference_tables(golden):
    """train_model()'s epoch of the golden through run_schedule from the resident sequences; the end tables under the
    trace's rule"""
    import torch
    from test_srgnn_cpu import golden_table
    g = golden
    d, step, nonhybrid, l2, L, _ = _case(g, "hybrid")
    from test_srgnn_cpu import case_init
    init = case_init(g, "epoch")
    eng = _engine(init, L, step, int(g["batch_epoch"]), float(g["lr"]), l2, nonhybrid)
    eng.set_sequences(g["seq_ptr"], g["seq"])
    S = len(g["epoch_users"])
    losses = torch.zeros((S, 2), device=eng.T["embedding"].device)
    eng.run_schedule(g["epoch_users"], g["epoch_ends"], losses, g["epoch_lrs"])
    assert eng.adam.t == S and np.isfinite(losses.cpu().numpy()).all()
    for name, got in _tables(eng).items():
        _close(got, golden_table(g, "epoch", name, 0, init), float(g["epoch_gap_" + name][0]), "epoch end %s" % name)


def test_predict_matches_the_reference(golden):
    """predict(), full and candidate mode, after the case `gated`, for a user count that is no multiple of the batch"""
    g = golden
    d, step, nonhybrid, l2, L, init = _case(g, "gated")
    eng = _engine(init, L, step, int(g["batch_step"]), float(g["lr"]), l2, nonhybrid)
    loss2 = _loss2(eng)
    for s in range(len(g["gated_seq"])):
        eng.step(g["gated_seq"][s], g["gated_target"][s], loss2, float(g["gated_lrs"][s]))
    eng.set_sequences(g["seq_ptr"], g["seq"])
    users, cand = g["predict_users"], g["predict_cand"]
    assert len(users) % int(g["batch_step"])
    got = eng.score(users)
    assert got.is_cuda and tuple(got.shape) == (len(users), eng.n_items)
    got = got.cpu().numpy()
    _close(got, g["predict_f64"], np.abs(g["predict_f32"] - g["predict_f64"]).max(), "predict")
    got_c = np.stack([got[k][c] for k, c in enumerate(cand)])
    _close(got_c, g["predict_cand_f64"], np.abs(g["predict_cand_f32"] - g["predict_cand_f64"]).max(),
           "predict, candidates")


# ------------------------------------------------------------------ edges of the step
def _batch(I, L, B, kind, seed):
    rs = np.random.RandomState(seed)
    seq = np.full((B, L), I, np.int32)
    for b in range(B):
        n = {"equal": L, "ramp": 1 + b % L, "distinct": L, "same": L}.get(kind, rs.randint(1, L + 1))
        if kind == "distinct":
            seq[b, :n] = rs.permutation(I)[:n]
        elif kind == "same":
            seq[b, :n] = rs.randint(0, I)
        else:
            seq[b, :n] = rs.randint(0, I, n)
    target = rs.randint(0, I, B).astype(np.int32)
    target[0] = 0                                                    # target 0 and target I - 1
    target[-1] = I - 1 if B > 1 else 0
    return seq, target


def _check_gradients(tab, seq, target, L, step, nonhybrid, l2):
    """gradients() against the float64 restatement: per tensor within 4x the float32 restatement's distance from the
    float64 one at the same inputs, plus 1e-5 max|want|.  Adam is left out on purpose: its first step is lr sign(g) and
    hides the size of an error."""
    eng = _engine(tab, L, step, len(seq), 0.001, l2, nonhybrid)
    before = _tables(eng)
    loss2 = _loss2(eng)
    eng.gradients(seq, target, loss2)
    ce64, reg64, G64 = P.loss_and_grads(tab, seq, target, step, l2, nonhybrid, np.float64)
    ce32, reg32, G32 = P.loss_and_grads(tab, seq, target, step, l2, nonhybrid, np.float32)
    got = loss2.cpu().numpy().astype(np.float64)
    _close(got[:1], np.asarray([ce64]), abs(float(ce32) - ce64), "cross-entropy")
    _close(got[1:], np.asarray([reg64]), abs(float(reg32) - reg64), "regulariser")
    for name in P.NAMES:
        g = eng.G[name].cpu().numpy()
        assert np.isfinite(g).all(), name
        _close(g, G64[name], np.abs(G32[name].astype(np.float64) - G64[name]).max(), name)
    for name, t in _tables(eng).items():                            # gradients() moves no table
        assert np.array_equal(t, before[name]), name
    assert eng.guard_row.eq(eng.guard_row[0]).all().item() and eng.guard_row[0].item() == 12345.0
    return eng


@pytest.mark.parametrize("d,I,L,B,step,nonhybrid,kind", [
    (20, 131, 6, 1, 1, False, "mixed"),         # B = 1
    (64, 64, 7, 5, 4, False, "equal"),          # a batch of equal lengths, four iterations
    (65, 65, 9, 9, 1, True, "ramp"),            # lengths 1 to L mixed
    (8, 300, 256, 2, 1, False, "distinct"),     # the longest session, all items distinct
    (4, 63, 256, 2, 4, True, "same"),           # the longest session, one item throughout: one node, a self-loop
    (128, 131, 5, 3, 1, True, "mixed"),         # the widest row
    (1, 1, 4, 3, 4, False, "mixed"),            # d = 1, one item
    (20, 63, 12, 70, 1, False, "mixed"),        # more sessions than chunks of the variable gradients
])
def test_gradients_at_the_edge_shapes(d, I, L, B, step, nonhybrid, kind):
    tab = P.init_tables(I, d, seed=d + L)
    seq, target = _batch(I, L, B, kind, seed=B + L)
    _check_gradients(tab, seq, target, L, step, nonhybrid, l2=0.01)


def test_saturated_logits():
    """the table scaled by 50: the logits reach hundreds, the softmax is one-hot or nearly; the loss and every gradient
    are finite and meet the restatement, which subtracts the row maximum as TF does"""
    d, I, L, B = 16, 65, 6, 7
    tab = P.init_tables(I, d, seed=3, scale=50.0)
    seq, target = _batch(I, L, B, "mixed", seed=11)
    assert np.abs(P.logits(tab, seq, 1)).max() > 100
    _check_gradients(tab, seq, target, L, 1, False, l2=1e-5)


def test_guard_row_and_zero_buffers_after_short_sessions():
    """sessions far shorter than max_seq_len: the pad id is no node, so the row behind the table is never written; the
    gradient buffers are zero after each step"""
    d, I, L, B = 20, 63, 16, 9
    tab = P.init_tables(I, d, seed=5)
    eng = _engine(tab, L, 2, B, l2=1e-5)
    loss2 = _loss2(eng)
    for s in range(3):
        seq, target = _batch(I, L, B, "ramp", seed=s)
        seq[:, 3:] = I
        eng.step(seq, target, loss2)
        assert np.isfinite(loss2.cpu().numpy()).all()
        for name, G in eng.G.items():
            assert not G.any().item(), name
        assert eng.guard_row.eq(12345.0).all().item()
    assert not np.array_equal(_tables(eng)["embedding"], tab["embedding"])


def test_two_engines_are_bit_identical_after_three_steps():
    d, I, L, B = 64, 131, 20, 33
    tab = P.init_tables(I, d, seed=4)
    runs = []
    for _ in range(2):
        eng = _engine(tab, L, 2, B, l2=1e-5)
        loss2 = _loss2(eng)
        losses = []
        for s in range(3):
            seq, target = _batch(I, L, B, "mixed", seed=40 + s)
            eng.step(seq, target, loss2, 0.001 * 0.5 ** s)
            losses.append(loss2.cpu().numpy().copy())
        runs.append((_tables(eng), losses))
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
    assert np.array_equal(np.stack(runs[0][1]), np.stack(runs[1][1]))


def test_pairs_over_resident_sequences_equal_padded_rows():
    """the (user, end) form gathers the same windows on the device as the padded rows hold: identical gradients"""
    d, I, L = 20, 63, 5
    tab = P.init_tables(I, d, seed=6)
    rs = np.random.RandomState(2)
    counts = np.asarray([0, 1, 2, 5, 9, 3])
    seq_ptr = np.concatenate([[0], np.cumsum(counts)])
    flat = rs.randint(0, I, counts.sum()).astype(np.int32)
    users = np.asarray([2, 3, 4, 4, 5], np.int32)
    ends = np.asarray([1, 4, 8, 2, 2], np.int32)
    seq = np.full((len(users), L), I, np.int32)
    target = np.zeros(len(users), np.int32)
    for k, (u, e) in enumerate(zip(users, ends)):
        row = flat[seq_ptr[u]:seq_ptr[u + 1]]
        cut = row[max(0, e - L):e]
        seq[k, :len(cut)] = cut
        target[k] = row[e]
    a, b = _engine(tab, L, 1, 8, l2=1e-5), _engine(tab, L, 1, 8, l2=1e-5)
    la, lb = _loss2(a), _loss2(b)
    a.step(seq, target, la)
    b.set_sequences(seq_ptr, flat)
    b.run_schedule(users[None], ends[None], lb[None])
    assert np.array_equal(la.cpu().numpy(), lb.cpu().numpy())
    for k, t in _tables(a).items():
        assert np.array_equal(t, _tables(b)[k]), k
    with pytest.raises(ValueError, match="an end without a target"):
        b.run_schedule(users[None], np.asarray([[2, 4, 8, 2, 2]]), lb[None])


def test_score_batches_and_a_user_without_items():
    """six users through max_batch 4 take two forward calls; the rows equal the restatement's logits; a user without
    items, or outside the data, scores a zero row"""
    d, I, L = 20, 70, 5
    tab = P.init_tables(I, d, seed=7)
    eng = _engine(tab, L, 2, 4)
    with pytest.raises(ValueError, match="set_sequences"):
        eng.score([0])
    rs = np.random.RandomState(3)
    counts = np.asarray([3, 0, 7, 1, 5, 2])
    seq_ptr = np.concatenate([[0], np.cumsum(counts)])
    flat = rs.randint(0, I, counts.sum()).astype(np.int32)
    eng.set_sequences(seq_ptr, flat)
    got = eng.score(np.arange(6))
    assert eng.forward_calls == 2 and got.is_cuda and tuple(got.shape) == (6, I)
    got = got.cpu().numpy()
    seq = np.full((6, L), I, np.int32)
    for u in range(6):
        cut = flat[seq_ptr[u]:seq_ptr[u + 1]][-L:]
        seq[u, :len(cut)] = cut
    want = P.logits(tab, seq, 2)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert not got[1].any() and np.abs(got[0]).max() > 0
    assert not eng.score([9]).cpu().numpy().any()
    rows = eng.forward_rows(seq).cpu().numpy()
    want_rows = P.forward(tab, seq, 2)
    assert np.abs(rows - want_rows).max() <= 1e-5 * np.abs(want_rows).max()


def test_refusals():
    tab = P.init_tables(9, 4, seed=1)
    for kw, text in ((dict(L=257), r"max_seq_len=257 is not supported \(1 to 256\)"),
                     (dict(step=5), r"step=5 is not supported \(1 to 4\)"),
                     (dict(step=0), r"step=0 is not supported \(1 to 4\)"),
                     (dict(max_batch=4097), r"batch_size=4097 is not supported \(1 to 4096\)")):
        args = dict(L=5, step=1, max_batch=4)
        args.update(kw)
        with pytest.raises(NotImplementedError, match=text):
            _engine(tab, args["L"], args["step"], args["max_batch"])
    with pytest.raises(NotImplementedError, match=r"hidden_size=129 is not supported \(1 to 128\)"):
        _engine(P.init_tables(9, 129, seed=1), 5, 1, 4)
    wide = dict(tab)
    wide["embedding"] = np.zeros((1 << 19, 4), np.float32)
    with pytest.raises(NotImplementedError, match=r"batch_size \* num_items = 2147483648 is not supported"):
        _engine(wide, 5, 1, 4096)
    # the C entry refuses by name too
    import ctypes as C
    from neurec_amd._lib import call
    floats = C.c_size_t(0)
    for shape, text in (((4, 257, 8, 1, 9), "max_seq_len 257 outside"), ((4, 5, 129, 1, 9), "hidden_size 129 outside"),
                        ((4, 5, 8, 5, 9), "step 5 outside"), ((4097, 5, 8, 1, 9), "batch_size 4097 outside"),
                        ((4096, 5, 8, 1, 1 << 19), "batch_size \\* num_items")):
        with pytest.raises(NotImplementedError, match=text):
            call("nrhip_srgnn_workspace_floats", *shape, C.byref(floats))
    eng = _engine(tab, 5, 1, 2)
    loss2 = _loss2(eng)
    seq, target = _batch(9, 5, 3, "mixed", seed=1)
    with pytest.raises(ValueError, match="batch larger than max_batch"):
        eng.step(seq, target, loss2)
    with pytest.raises(ValueError, match=r"seq holds an id outside \[0, 9\]"):
        eng.step(np.full((2, 5), 10), target[:2], loss2)
    with pytest.raises(ValueError, match=r"target holds an id outside \[0, 9\)"):
        eng.step(seq[:2], np.asarray([9, 0]), loss2)
    assert eng.adam.t == 0


# ------------------------------------------------------------------ the drop-in run
def test_srgnn_config_drops_in(tmp_path):
    """NeuRec.properties + conf/SRGNN.properties (the reference's values) on ml-100k with by_time=True: two epochs
    through neurec_amd.main; the metrics header, the deviation line and two `epoch` lines, in order; predict()'s modes"""
    from neurec_amd.model.sequential_recommender.SRGNN import DEVIATIONS
    model = _run(tmp_path, ["--recommender=SRGNN", "--epochs=2", "--max_seq_len=20"])
    eng = model.engine
    assert (eng.d, eng.L, eng.S, eng.max_batch, eng.nonhybrid, eng.L2) == (64, 20, 1, 100, False, 1e-5)
    assert eng.adam.t == model.global_step > 0
    folder = os.path.join(str(tmp_path), "log", "ml-100k", "SRGNN")
    files = os.listdir(folder)
    assert len(files) == 1
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "SRGNN's hyperparameters:" in text
    lines = [ln for ln in text.splitlines() if re.search(r"metrics:\t|epoch \d+:\t", ln) or DEVIATIONS in ln]
    kinds = ["m" if "metrics:" in ln else "d" if DEVIATIONS in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)
             for ln in lines]
    assert kinds == ["m", "d", "e0", "e1"], kinds
    shown = np.asarray([float(x) for x in re.findall(r"epoch 1:\t(.+)", text)[0].split()])
    assert np.all(np.isfinite(shown)) and shown.max() > 0
    full = model.predict([0, 5, 9], None)
    assert tuple(full.shape) == (3, model.num_item) and full.is_cuda
    full = full.cpu().numpy()
    assert np.isfinite(full).all()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])
    assert np.array_equal(cand[1], full[1][[7]])


def test_plugin_refusals(tmp_path, monkeypatch):
    with pytest.raises(NotImplementedError, match=r"max_seq_len=300 is not supported \(1 to 256\)"):
        _run(tmp_path, ["--recommender=SRGNN", "--epochs=1", "--max_seq_len=300"])
    with pytest.raises(NotImplementedError, match=r"step=5 is not supported \(1 to 4\)"):
        _run(tmp_path, ["--recommender=SRGNN", "--epochs=1", "--step=5"])
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)                                # WORLD_SIZE > 1
    with pytest.raises(NotImplementedError, match="SRGNN runs on one GPU"):
        _run(tmp_path, ["--recommender=SRGNN", "--epochs=1"])
