"""ConvNCF on the GPU (csrc/convncf.hip through neurec_amd/convncf.py): every step of the reference class's trace (run
twice, bit for bit), the recorded epoch, predict() in both modes; on the shapes no golden holds the step's gradients, the
losses, the Adagrad forms, the all-items scorer and the pairs against the float64 restatement, allowed 4 x the distance
between the restatement's own float32 and float64 forms plus 1e-5 max|want|; the marker cases; empty work; the host
checks; the drop-in run through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import convncf_restatement as P
from convncf_restatement import CASES
from test_convncf_cpu import (MARKER_CASES, case_feeds, case_init, check_marker_scores, golden_table, marker_corners,
                              marker_tables, saturated_point, small_batch, transpose_point, zero_pre_activation_point)
from test_gru4rec_gpu import _close, _run

pytestmark = pytest.mark.gpu
REGS = (0.01, 0.02, 0.03)


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_convncf")


def _engine(tab, max_batch, loss="bpr", regs=(0.0, 0.0, 0.0), lr_embed=0.05, lr_net=0.1):
    from neurec_amd.convncf import ConvNCFEngine
    channels = [tab["kernel%d" % k].shape[3] for k in range(P.n_layers_of(tab))]
    return ConvNCFEngine(tab, channels, lr_embed, lr_net, regs, max_batch, loss=loss)


def _case_engine(g, case, init=None, batch=None):
    d, channels, loss, regs, lr_embed, lr_net, _ = CASES[P.EPOCH_CASE if case == "epoch" else case]
    init = case_init(g, case) if init is None else init
    return _engine(init, int(g["batch_step"]) if batch is None else batch, loss, regs, lr_embed, lr_net), init


def _tables(eng):
    return {k: t.cpu().numpy() for k, t in eng.tables().items()}


def _loss2(eng):
    import torch
    return torch.zeros(2, device=eng.T["embedding_P"].device)


def _clean(eng):
    for name, G in eng.G.items():
        assert not G.any().item(), name
    for name, flag in eng.flag.items():
        assert not flag.any().item(), name


def _near(got, want, want32, what):
    """the edge shapes' rule: 4 x |the restatement's float32 form - its float64 form| + 1e-5 max|want|"""
    _close(np.asarray(got), np.asarray(want, np.float64), np.abs(np.asarray(want32, np.float64) - want).max(initial=0), what)


# ------------------------------------------------------------------ the reference's trace
@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace_and_rerun_to_the_same_bits(golden, case):
    """Every variable after every step, and each step's loss, against the f64 trace: within 4x the reference's own
    f32-to-f64 distance of that step and tensor (read from the golden) plus 1e-5 max|want|.  The gradient buffers and
    the row flags are zero again afterwards.  A second engine on the same feeds ends on the same bits."""
    g = golden
    runs = []
    for rerun in range(2):
        eng, init = _case_engine(g, case)
        assert list(eng.tables()) == P.names(len(CASES[case][1]))
        loss2, seen = _loss2(eng), []
        for s, (users, pos, neg) in enumerate(case_feeds(g, case)):
            eng.step(users, pos, neg, loss2)
            seen.append(loss2.cpu().numpy().copy())
            if rerun:
                continue
            l64, l32 = float(g[case + "_loss_f64"][s]), float(g[case + "_loss_f32"][s])
            _close(np.asarray([loss2[0].item()]), np.asarray([l64]), abs(l32 - l64), "%s step %d loss" % (case, s + 1))
            for name, got in _tables(eng).items():
                _close(got, golden_table(g, case, name, s, init)[0], float(g["%s_gap_%s" % (case, name)][s]),
                       "%s step %d %s" % (case, s + 1, name))
            _clean(eng)
        assert eng.t == CASES[case][6]
        runs.append((_tables(eng), np.stack(seen), {k: a.cpu().numpy() for k, a in eng.acc.items()}))
    assert all(np.array_equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0])
    assert np.array_equal(runs[0][1], runs[1][1])
    assert all(np.array_equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])


def test_the_recorded_epoch_ends_at_the_reference_tables(golden):
    """train_model()'s epoch of the golden, batch by batch in the order the class was fed, the last batch cut to its
    true size; the end tables under the trace's rule"""
    import torch
    g = golden
    eng, init = _case_engine(g, "epoch", batch=int(g["batch_epoch"]))
    dev = eng.T["embedding_P"].device
    users, pos, neg = (torch.from_numpy(g["epoch_" + k]).to(dev) for k in ("users", "pos", "neg"))
    rows = g["epoch_rows"]
    losses = torch.zeros((len(rows), 2), device=dev)
    for s, n in enumerate(rows):
        eng.step(users[s, :n], pos[s, :n], neg[s, :n], losses[s])
    assert eng.t == len(rows) and np.isfinite(losses.cpu().numpy()).all()
    for name, got in _tables(eng).items():
        _close(got, golden_table(g, "epoch", name, 0, init)[0], float(g["epoch_gap_" + name][0]), "epoch end %s" % name)


@pytest.mark.parametrize("case", P.PREDICT_CASES)
def test_predict_matches_the_reference(golden, case):
    """predict(), full and candidate mode, after the case's last step, under the trace's rule"""
    from neurec_amd.model.general_recommender.ConvNCF import predict_pairs
    g = golden
    eng, _ = _case_engine(g, case)
    loss2 = _loss2(eng)
    for users, pos, neg in case_feeds(g, case):
        eng.step(users, pos, neg, loss2)
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
def _batch(U, I, B, seed):
    rs = np.random.RandomState(seed)
    return tuple(rs.randint(0, n, B).astype(np.int32) for n in (U, I, I))


def _check_gradients(tab, users, pos, neg, loss, regs, max_batch):
    eng = _engine(tab, max_batch, loss, regs)
    loss2 = _loss2(eng)
    eng.gradients(users, pos, neg, loss2)
    (term, reg), want = P.gradients(tab, users, pos, neg, loss, regs)
    (term32, reg32), want32 = P.gradients(tab, users, pos, neg, loss, regs, np.float32)
    got2 = loss2.cpu().numpy()
    _near([got2[0]], [term], [term32], "loss")
    _near([got2[1]], [reg], [reg32], "regulariser")
    for name, w in want.items():
        _near(eng.G[name].cpu().numpy(), w, want32[name], name)
    assert eng.t == 0 and all(np.array_equal(v, tab[k]) for k, v in _tables(eng).items())     # no variable moved
    assert all((a == np.float32(0.1)).all().item() for a in eng.acc.values())
    assert np.array_equal(np.flatnonzero(eng.flag["embedding_P"].cpu().numpy()), np.unique(users))
    assert np.array_equal(np.flatnonzero(eng.flag["embedding_Q"].cpu().numpy()), np.unique(np.concatenate([pos, neg])))
    return eng, want


# (d, net_channel, batch, loss): batch 1; 4,096 at d = 4; channel counts 1, 31, 32 (the largest); more than one block
# of the outer product (d = 64); every loss
GRADIENT_CASES = [(4, [3, 5], 1, "bpr"), (4, [3, 5], 4096, "hinge"), (2, [1], 20, "square"), (2, [32], 20, "bpr"),
                  (8, [31, 32, 1], 20, "bpr"), (16, [32, 31, 1, 32], 9, "hinge"), (32, [1, 31, 32, 2, 3], 7, "square"),
                  (64, [3, 32, 5, 31, 2, 4], 5, "hinge")]


@pytest.mark.parametrize("d,channels,B,loss", GRADIENT_CASES)
def test_gradients_equal_the_restatement(d, channels, B, loss):
    U, I = 23, 29
    tab = P.init_tables(U, I, d, channels, seed=len(channels) * 131 + d)
    users, pos, neg = _batch(U, I, B, B + d)
    _check_gradients(tab, users, pos, neg, loss, REGS, max(B, 2))


def test_gradients_with_repeats_of_every_kind():
    """a repeated user, an item positive here and negative there, a triplet given twice, and one user for a whole batch"""
    U, I = 9, 11
    tab = P.init_tables(U, I, 8, [4, 8, 6], seed=12)
    users, pos, neg = small_batch(U, I, 12, 1)
    _check_gradients(tab, users, pos, neg, "bpr", REGS, 12)
    _check_gradients(tab, np.full(12, users[0], np.int32), pos, neg, "square", REGS, 12)


def test_gradients_where_a_layer_s_pre_activations_are_all_exactly_zero():
    tab, (u, i, j) = zero_pre_activation_point()
    _, want = _check_gradients(tab, u, i, j, "bpr", (0.0, 0.0, 0.0), 8)
    assert want["kernel1"].any() and not want["kernel0"].any() and not want["W"].any()


def test_a_saturated_tanh_passes_a_gradient_of_zero_not_nan():
    tab, (u, i, j) = saturated_point()
    eng, want = _check_gradients(tab, u, i, j, "square", (0.0, 0.0, 0.0), 8)
    assert all(np.isfinite(G.cpu().numpy()).all() for G in eng.G.values())
    for name in ("kernel0", "bias0", "embedding_P", "embedding_Q"):
        assert not eng.G[name].any().item(), name
    assert want["kernel1"].any() and eng.G["kernel1"].any().item()


# ------------------------------------------------------------------ the step: losses, Adagrad, clean buffers
@pytest.mark.parametrize("loss", ["bpr", "hinge", "square"])
def test_two_steps_in_every_loss_form(loss):
    """each step's loss and every variable against the restatement's State; the tables move by lr_embed, the dense
    variables by lr_net; the buffers and flags are zero after each step"""
    U, I = 23, 29
    tab = P.init_tables(U, I, 8, [4, 8, 6], seed=21)
    eng = _engine(tab, 20, loss, REGS, lr_embed=0.03, lr_net=0.2)
    st = {dt: P.State(tab, loss, REGS, 0.03, 0.2, dt) for dt in (np.float64, np.float32)}
    loss2 = _loss2(eng)
    for s in range(2):
        users, pos, neg = _batch(U, I, 20, 40 + s)
        eng.step(users, pos, neg, loss2)
        (t64, r64), (t32, r32) = (st[dt].step(users, pos, neg) for dt in (np.float64, np.float32))
        got2 = loss2.cpu().numpy()
        _near([got2[0]], [t64], [t32], "%s step %d loss" % (loss, s + 1))
        _near([got2[1]], [r64], [r32], "%s step %d regulariser" % (loss, s + 1))
        for name, got in _tables(eng).items():
            _near(got, st[np.float64].var[name], st[np.float32].var[name], "%s step %d %s" % (loss, s + 1, name))
            _near(eng.acc[name].cpu().numpy(), st[np.float64].acc[name], st[np.float32].acc[name], "accumulator " + name)
        _clean(eng)
    assert eng.t == 2


def test_adagrad_keeps_what_the_batch_did_not_touch():
    """a row touched in step 1 and not in step 2 keeps its accumulator and value in step 2; an untouched row's
    accumulator stays exactly 0.1; one step moves a table entry by lr_embed g / sqrt(0.1 + g^2), a dense one by lr_net"""
    U, I = 9, 11
    tab = P.init_tables(U, I, 4, [3, 2], seed=4)
    regs = (0.01, 0.0, 0.0)
    eng = _engine(tab, 8, "bpr", regs, lr_embed=0.05, lr_net=0.2)
    u, i, j = small_batch(U, I, 8, 5)
    _, G = P.gradients(tab, u, i, j, "bpr", regs)
    loss2 = _loss2(eng)
    eng.step(u, i, j, loss2)
    T1, A1 = _tables(eng), {k: a.cpu().numpy() for k, a in eng.acc.items()}
    rest = np.setdiff1d(np.arange(U), u)
    assert len(rest) and (A1["embedding_P"][rest] == np.float32(0.1)).all()
    assert np.array_equal(T1["embedding_P"][rest], tab["embedding_P"][rest])
    rest = np.setdiff1d(np.arange(I), np.concatenate([i, j]))
    assert len(rest) and (A1["embedding_Q"][rest] == np.float32(0.1)).all()
    g = G["embedding_P"][u[0]]
    want = tab["embedding_P"][u[0]] - 0.05 * g / np.sqrt(0.1 + g * g)
    assert np.abs(T1["embedding_P"][u[0]] - want).max() <= 1e-5 * np.abs(want).max()
    assert np.abs(T1["embedding_P"][u[0]] - tab["embedding_P"][u[0]]).max() > 1e-3     # lr_net would be 4 x as far
    want = tab["W"] - 0.2 * G["W"] / np.sqrt(0.1 + G["W"] ** 2)
    assert np.abs(T1["W"] - want).max() <= 1e-5 * np.abs(want).max()
    others = np.where(u == u[0], (u[0] + 1) % U, u).astype(np.int32)
    eng.step(others, i, j, loss2)
    T2, A2 = _tables(eng), {k: a.cpu().numpy() for k, a in eng.acc.items()}
    assert u[0] not in others and np.array_equal(A2["embedding_P"][u[0]], A1["embedding_P"][u[0]])
    assert np.array_equal(T2["embedding_P"][u[0]], T1["embedding_P"][u[0]])
    assert not np.array_equal(T2["embedding_Q"][i[0]], T1["embedding_Q"][i[0]])
    _clean(eng)


def test_an_empty_batch_is_a_no_op():
    import torch
    U, I = 9, 11
    tab = P.init_tables(U, I, 4, [3, 2], seed=1)
    eng = _engine(tab, 8, regs=REGS)
    loss2 = torch.ones(2, device=eng.T["embedding_P"].device)
    empty = np.zeros(0, np.int32)
    eng.step(empty, empty, empty, loss2)
    assert eng.t == 0 and (loss2 == 1.0).all().item()               # no buffer is touched, loss_out included
    assert all(np.array_equal(v, tab[k]) for k, v in _tables(eng).items())
    assert all((a == np.float32(0.1)).all().item() for a in eng.acc.values())
    assert tuple(eng.score(empty).shape) == (0, I) and eng.forward([], []).numel() == 0
    _clean(eng)
    assert eng.workspace_floats(0) > 0 and eng.workspace_floats() >= eng.workspace_floats(1)


# ------------------------------------------------------------------ the all-items scorer and the pairs
def _check_scores(tab, users, guard=True):
    import torch
    eng = _engine(tab, 8)
    I, n = len(tab["embedding_Q"]), len(users)
    want, want32 = P.scores(tab, users), P.scores(tab, users, np.float32)
    if guard:
        out = torch.full((n + 1, I + 3), -7.5, device=eng.T["embedding_P"].device)
        got = eng.score(users, out=out)
        whole = out.cpu().numpy()
        assert (whole[n:] == -7.5).all() and (whole[:, I:] == -7.5).all()     # the canaries behind the output
    else:
        got = eng.score(users)
    assert got.is_cuda and tuple(got.shape) == (n, I)
    got = got.cpu().numpy()
    _near(got, want, want32, "scores")
    return eng, got, want, want32


@pytest.mark.parametrize("d,channels", [(4, [3, 5]), (16, [4, 8, 8, 6])])
@pytest.mark.parametrize("I", [1, 31, 32, 33, 131])
@pytest.mark.parametrize("n", [1, 7, 33])
def test_scores_at_every_item_and_user_count(d, channels, I, n):
    U = 40
    tab = P.init_tables(U, I, d, channels, seed=I + n)
    users = np.random.RandomState(n).randint(0, U, n).astype(np.int32)
    _check_scores(tab, users)


@pytest.mark.parametrize("d,channels", [(2, [3]), (8, [31, 32, 1]), (32, [1, 31, 32, 2, 3]), (64, [32] * 6)])
def test_scores_and_pairs_agree_on_every_depth(d, channels):
    """users out of order and one given twice; forward(users, items) gives the same entries as score(users); at d = 64
    8 users x 131 items against the restatement"""
    U, I = 11, 131 if d == 64 else 45
    tab = P.init_tables(U, I, d, channels, seed=sum(channels) + d)
    users = np.asarray([9, 0, 10, 3, 3, 7, 1, 2], np.int32)
    eng, got, want, want32 = _check_scores(tab, users)
    assert np.array_equal(got[3], got[4])
    rs = np.random.RandomState(1)
    pu, pi = rs.randint(0, len(users), 50), rs.randint(0, I, 50).astype(np.int32)
    pairs = eng.forward(users[pu], pi).cpu().numpy()
    assert np.array_equal(pairs, got[pu, pi])                      # one forward path for both
    _near(pairs, want[pu, pi], want32[pu, pi], "pairs")


def test_scores_beyond_the_largest_grid_of_one_launch():
    """4,097 users x 4,097 items is more than 2^24 pairs, the most workgroups of 256 threads one launch can hold, and
    more than the 2^20 workgroups a launch here is given: every entry is written, rows from both ends and the middle
    against the restatement"""
    import torch
    U = I = 4097
    tab = P.init_tables(U, I, 2, [3], seed=6)
    eng = _engine(tab, 8)
    assert U * I > 1 << 24
    out = torch.full((U, I), float("nan"), device=eng.T["embedding_P"].device)
    got = eng.score(np.arange(U, dtype=np.int32), out=out)
    assert not torch.isnan(got).any().item()
    rows = np.asarray([0, 1, 255, 256, 2048, 4095, 4096])
    got = got[torch.from_numpy(rows).to(got.device)].cpu().numpy()
    _near(got, P.scores(tab, rows), P.scores(tab, rows, np.float32), "rows of 16.8 M scores")


def test_score_adds_the_output_bias():
    U, I = 5, 7
    tab = P.init_tables(U, I, 4, [3, 2], seed=2)
    tab["b"][:] = 3.0
    _, got, want, _ = _check_scores(tab, np.arange(U, dtype=np.int32))
    assert np.abs(got).min() > 1.0 and np.abs(want).min() > 1.0


# ------------------------------------------------------------------ marker cases
@pytest.mark.parametrize("L,k,corner", MARKER_CASES)
def test_a_corner_kernel_lights_one_pair_of_one_hot_rows(L, k, corner):
    """one-hot rows and kernels that pass one corner of every patch: every score is exactly b but one; the gradients of
    that pair's triplet against the restatement, where a wrong corner is a whole kernel slice, not ulps"""
    corners = marker_corners(L, k, corner)
    tab, u, i = marker_tables([2] * L, corners)
    d = 1 << L
    eng = _engine(tab, 4, "square")
    S = eng.score(np.arange(d, dtype=np.int32)).cpu().numpy()
    check_marker_scores(S, tab, u, i)
    users, pos, neg = np.asarray([u], np.int32), np.asarray([i], np.int32), np.asarray([(i + 1) % d], np.int32)
    eng.gradients(users, pos, neg, _loss2(eng))
    _, want = P.gradients(tab, users, pos, neg, "square")
    _, want32 = P.gradients(tab, users, pos, neg, "square", dtype=np.float32)
    for name, w in want.items():
        _near(eng.G[name].cpu().numpy(), w, want32[name], name)
    for n, c in enumerate(corners):
        g = eng.G["kernel%d" % n].cpu().numpy()
        assert g[c[0], c[1]].any()


def test_the_two_axes_of_the_outer_product_are_not_transposed():
    tab = transpose_point()
    _, got, want, _ = _check_scores(tab, np.arange(3, dtype=np.int32))
    swapped = dict(tab, embedding_P=tab["embedding_Q"], embedding_Q=tab["embedding_P"])
    assert np.abs(got - P.scores(swapped, np.arange(3)).T).max() > 0.05
    u, i, j = np.asarray([0, 1], np.int32), np.asarray([1, 2], np.int32), np.asarray([2, 0], np.int32)
    _check_gradients(tab, u, i, j, "bpr", REGS, 2)


# ------------------------------------------------------------------ host checks
def test_shapes_outside_the_kernels_are_refused_by_name():
    from neurec_amd.convncf import ConvNCFEngine
    U, I = 5, 7

    def make(d, channels, **kw):
        tab = P.init_tables(U, I, d, channels or [1], seed=1)
        tab = {k: v for k, v in tab.items() if k in P.names(len(channels))}
        return ConvNCFEngine(tab, channels, 0.05, 0.05, [0.0, 0.0, 0.0], kw.pop("max_batch", 8), **kw)
    for d, channels, text in ((8, [3, 5], r"embedding_size=8 is not supported with 2 layers"),
                              (2, [], r"net_channel=\[\] is not supported \(1 to 6 layers\)"),
                              (128, [2] * 7, r"is not supported \(1 to 6 layers\)"),
                              (4, [3, 33], r"net_channel\[1\]=33 is not supported \(1 to 32\)")):
        with pytest.raises(NotImplementedError, match=text):
            make(d, channels)
    tab = P.init_tables(U, I, 4, [3, 5], seed=1)
    with pytest.raises(NotImplementedError, match=r"net_channel\[0\]=0 is not supported \(1 to 32\)"):
        ConvNCFEngine(tab, [0, 5], 0.05, 0.05, [0.0, 0.0, 0.0], 8)
    with pytest.raises(NotImplementedError, match=r"batch_size=4097 is not supported \(1 to 4096\)"):
        make(4, [3, 5], max_batch=4097)
    with pytest.raises(Exception, match="please choose a suitable loss function"):
        make(4, [3, 5], loss="cross_entropy")


def test_ids_outside_the_tables_are_refused_on_the_host():
    U, I = 9, 11
    eng = _engine(P.init_tables(U, I, 4, [3, 2], seed=1), 8)
    loss2 = _loss2(eng)
    with pytest.raises(ValueError, match=r"ConvNCF: users holds an id outside \[0, 9\)"):
        eng.step([0, 9], [1, 2], [3, 4], loss2)
    with pytest.raises(ValueError, match=r"ConvNCF: pos holds an id outside \[0, 11\)"):
        eng.step([0, 1], [1, -1], [3, 4], loss2)
    with pytest.raises(ValueError, match=r"ConvNCF: neg holds an id outside \[0, 11\)"):
        eng.step([0, 1], [1, 2], [3, 11], loss2)
    with pytest.raises(ValueError, match=r"users holds an id outside"):
        eng.score([9])
    with pytest.raises(ValueError, match=r"items holds an id outside"):
        eng.forward([0], [11])
    with pytest.raises(ValueError, match="batch larger than max_batch"):
        eng.step(np.zeros(9, np.int32), np.zeros(9, np.int32), np.zeros(9, np.int32), loss2)
    with pytest.raises(ValueError, match="same length"):
        eng.step([0, 1], [1, 2], [1], loss2)
    assert eng.t == 0
    _clean(eng)


# ------------------------------------------------------------------ the drop-in run
def test_convncf_config_drops_in(tmp_path):
    """NeuRec.properties + conf/ConvNCF.properties on ml-100k at a small shape: two epochs through neurec_amd.main; the
    reference's log lines, the evaluator through both predict modes"""
    model = _run(tmp_path, ["--recommender=ConvNCF", "--epochs=2", "--embedding_size=8", "--net_channel=[4,8,4]"])
    eng = model.engine
    assert (eng.d, eng.channels, eng.max_batch, eng.loss, eng.lr_embed, eng.lr_net, eng.regs) == \
        (8, [4, 8, 4], 512, "bpr", 0.05, 0.05, [0.01, 0.0, 0.0])
    nnz = model.dataset.train_matrix.nnz
    assert eng.t == 2 * -(-nnz // 512)
    assert all((eng.T["bias%d" % k].cpu().numpy() != np.float32(0.1)).any() for k in range(3))    # they started there
    folder = os.path.join(str(tmp_path), "log", "ml-100k", "ConvNCF")
    files = os.listdir(folder)
    assert len(files) == 1
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "ConvNCF's hyperparameters:" in text and "load pretrained params unsuccessful!" in text
    for epoch in (1, 2):
        assert re.search(r"\[iter %d : loss : [0-9.]+, time: [0-9.]+\]" % epoch, text)
        shown = np.asarray([float(x) for x in re.findall(r"epoch %d:\t(.+)" % epoch, text)[0].split()])
        assert np.all(np.isfinite(shown)) and shown.max() > 0
    first = float(re.search(r"\[iter 1 : loss : ([0-9.]+)", text).group(1))
    assert 10.0 < first < 512 * np.log(2.0) * 1.5                  # a SUM over a batch (a mean would be near 0.7)
    assert text.index("load pretrained params unsuccessful!") < text.index("[iter 1 :") < text.index("epoch 1:\t")
    full = model.predict([0, 5, 9], None)
    assert tuple(full.shape) == (3, model.num_items) and full.is_cuda
    full = full.cpu().numpy()
    assert np.isfinite(full).all()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1]
    assert np.array_equal(cand[0], full[0][[1, 2, 3]]) and np.array_equal(cand[1], full[1][[7]])
