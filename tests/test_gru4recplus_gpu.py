"""GRU4RecPlus on the GPU (csrc/gru4recplus.hip through neurec_amd/gru4recplus.py): every step of the reference class's
trace with the fetched states, the recorded epoch through the plugin's feeds, the users' final states and predict(), the
edge shapes of the step on its gradients, awkward logits, ids outside the table, determinism, empty work, the refusals
and the drop-in run through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import gru4recplus_restatement as P
from gru4recplus_restatement import CASES
from test_gru4rec_cpu import golden_table
from test_gru4rec_gpu import _close, _i32, _run, _set_states, _tables, _u8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_gru4recplus")


def _engine(V, layers, max_batch, n_sample, loss="bpr_max", hact="tanh", fact="linear", lr=0.001, reg=0.0, bpr_reg=1.0):
    from neurec_amd.gru4recplus import GRU4RecPlusEngine
    cells = [tuple(V["%s%d" % (n, l)] for n in ("Wg", "bg", "Wc", "bc")) for l in range(len(layers))]
    return GRU4RecPlusEngine(V["E_in"], V["Q"], V["b"], cells, lr, reg, max_batch, loss=loss, hidden_act=hact,
                             final_act=fact, bpr_reg=bpr_reg, n_sample=n_sample)


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Every variable and the fetched states after every step against the f64 trace: within 4x the reference's own
    f32-to-f64 distance of that step and tensor (read from the golden) plus 1e-5 max|want|.  Rows of E_in, Q and b
    outside <case>_rows_* are bit-equal to their initial value; the gradient buffers are zero again afterwards; the
    reset slots' states are zero."""
    import torch
    g = golden
    loss, hact, fact, layers, reg, bpr_reg, n_sample = CASES[case]
    names = P.table_names(len(layers))
    B = int(g["batch_step"])
    eng = _engine({n: g["%s_init_%s" % (case, n)] for n in names}, layers, B, n_sample, loss, hact, fact,
                  float(g["lr"]), reg, bpr_reg)
    loss2 = torch.zeros(2, device=eng.E_in.device)
    for s in range(len(g[case + "_X"])):
        mask = g[case + "_reset"][s]
        eng.step(_i32(eng, g[case + "_X"][s]), _i32(eng, g[case + "_Y"][s]), loss2, _u8(eng, mask))
        for l in range(len(layers)):
            w64, w32 = (g["%s_%s_state%d" % (case, tag, l)][s] for tag in ("f64", "f32"))
            _close(eng.h_new[l][:B].cpu().numpy(), w64, np.abs(w32 - w64).max(), "%s step %d state %d" % (case, s + 1, l))
            now = eng.states[l][:B].cpu().numpy()
            assert not now[mask].any() and np.array_equal(now[~mask], eng.h_new[l][:B].cpu().numpy()[~mask])
        for name, got in _tables(eng).items():
            w64, w32 = (golden_table(g, case, tag, name, s) for tag in ("f64", "f32"))
            _close(got, w64, np.abs(w32 - w64).max(), "%s step %d %s" % (case, s + 1, name))
            if name in ("E_in", "Q", "b"):
                still = np.setdiff1d(np.arange(len(got)), g["%s_rows_%s" % (case, name)])
                assert len(still) and np.array_equal(got[still], g["%s_init_%s" % (case, name)][still]), (case, s, name)
    assert np.isfinite(loss2.cpu().numpy()).all()
    for name, G in eng.G.items():                              # the gradient buffers are zero again
        assert not G.any().item(), name


def test_the_recorded_epoch_ends_at_the_reference_tables(golden):
    """train_model()'s epoch of the golden: the plugin's feeds from the recorded seed (bit-equal to the recorded ones)
    through run_schedule; the end tables under the trace's rule"""
    import torch
    from neurec_amd.model.sequential_recommender.GRU4RecPlus import epoch_feeds
    g = golden
    loss, hact, fact, layers, reg, bpr_reg, _ = CASES[P.PREDICT_CASE]
    names = P.table_names(len(layers))
    B, n = int(g["batch_epoch"]), int(g["n_sample_epoch"])
    np.random.seed(int(g["epoch_seed"]))
    X, Y, reset = epoch_feeds(g["offset_idx"], g["data_uit"][:, 1], g["pop_cumsum"], B, n)
    assert np.array_equal(X, g["epoch_X"]) and np.array_equal(Y, g["epoch_Y"])
    eng = _engine({k: g["epoch_init_" + k] for k in names}, layers, B, n, loss, hact, fact, float(g["lr"]), reg, bpr_reg)
    losses = torch.zeros((len(X), 2), device=eng.E_in.device)
    eng.run_schedule(X, Y, reset, losses)
    assert eng.t == len(g["epoch_X"]) and np.isfinite(losses.cpu().numpy()).all()
    for name, got in _tables(eng).items():
        w64, w32 = (golden_table(g, "epoch", tag, name, 0) for tag in ("f64", "f32"))
        _close(got, w64, np.abs(w32 - w64).max(), "epoch end %s" % name)


def test_user_states_and_predict_match_the_reference(golden):
    """_get_user_embeddings() and predict(), full and candidate mode, after the trained case, under the trace's rule"""
    import torch
    g = golden
    case = P.PREDICT_CASE
    loss, hact, fact, layers, reg, bpr_reg, n_sample = CASES[case]
    names = P.table_names(len(layers))
    B = int(g["batch_step"])
    eng = _engine({n: g["%s_init_%s" % (case, n)] for n in names}, layers, B, n_sample, loss, hact, fact,
                  float(g["lr"]), reg, bpr_reg)
    loss2 = torch.zeros(2, device=eng.E_in.device)
    for s in range(len(g[case + "_X"])):
        eng.step(_i32(eng, g[case + "_X"][s]), _i32(eng, g[case + "_Y"][s]), loss2, _u8(eng, g[case + "_reset"][s]))
    eng.set_sequences(g["seq_ptr"], g["seq"])
    H = eng.user_states().cpu().numpy()
    _close(H, g["user_emb_f64"], np.abs(g["user_emb_f32"] - g["user_emb_f64"]).max(), "user states")
    users, cand = g["predict_users"], g["predict_cand"]
    got = eng.score(users).cpu().numpy()
    _close(got, g["predict_f64"], np.abs(g["predict_f32"] - g["predict_f64"]).max(), "predict")
    got_c = np.stack([got[k][c] for k, c in enumerate(cand)])
    _close(got_c, g["predict_cand_f64"], np.abs(g["predict_cand_f32"] - g["predict_cand_f64"]).max(),
           "predict, candidates")


# ------------------------------------------------------------------ edges of the step
def _check_gradients(layers, B, n_sample, loss, hact, fact, reg=0.01, bpr_reg=0.7, I=50, X=None, Y=None, V=None,
                     zero_state=False, seed=0):
    """gradients() and the new states against the float64 restatement, 1e-5 max|want| per tensor (fp32 sums of at most
    a few hundred O(1) terms).  Adam is left out on purpose, as in test_gru4rec_gpu.py: its first step is lr sign(g) and
    hides the size of an error.  An id outside [0, I) is restated as an appended row of zeros whose gradient is dropped."""
    import torch
    rs = np.random.RandomState(seed)
    V = P.init_tables(I, layers, seed=seed + 1) if V is None else V
    eng = _engine(V, layers, B, n_sample, loss, hact, fact, reg=reg, bpr_reg=bpr_reg)
    X = rs.randint(I, size=B) if X is None else np.asarray(X)
    Y = rs.randint(I, size=B + n_sample) if Y is None else np.asarray(Y)
    states = [np.zeros((B, n), np.float32) if zero_state else (0.5 * rs.randn(B, n)).astype(np.float32) for n in layers]
    _set_states(eng, states)
    loss2 = torch.zeros(2, device=eng.E_in.device)
    before = _tables(eng)
    eng.gradients(_i32(eng, X), _i32(eng, Y), loss2)
    V64 = {k: v.astype(np.float64) for k, v in V.items()}
    for k in ("E_in", "Q", "b"):
        V64[k] = np.concatenate([V64[k], np.zeros((1,) + V64[k].shape[1:])])
    inside = lambda a: np.where((a >= 0) & (a < I), a, I)
    (lt, lr_), G, hs = P.gradients(V64, inside(X), inside(Y), [s.astype(np.float64) for s in states], loss, hact, fact,
                                   reg, bpr_reg)
    got2 = loss2.cpu().numpy().astype(np.float64)
    print("loss %.6g (want %.6g), regulariser %.6g (want %.6g)" % (got2[0], lt, got2[1], lr_))
    assert np.isfinite(got2).all()
    assert abs(got2[0] - lt) <= 1e-5 * abs(lt) and abs(got2[1] - lr_) <= 1e-5 * abs(lr_), (got2, lt, lr_)
    for l in range(len(layers)):
        err = np.abs(eng.h_new[l][:B].cpu().numpy() - hs[l]).max()
        assert err <= 1e-5 * np.abs(hs[l]).max(), ("state", l, err)
        assert np.array_equal(eng.states[l][:B].cpu().numpy(), states[l])          # gradients() moves no state
    for name, want in G.items():
        want = want[:I] if name in ("E_in", "Q", "b") else want
        got = eng.G[name].cpu().numpy()
        err = np.abs(got - want).max()
        print("%s: err %.3g, max|want| %.3g" % (name, err, np.abs(want).max()))
        assert np.isfinite(got).all() and err <= 1e-5 * np.abs(want).max(), (name, err, np.abs(want).max())
    for name, t in _tables(eng).items():                                           # and no table
        assert np.array_equal(t, before[name]), name
    return eng


@pytest.mark.parametrize("layers,B,n_sample,loss,hact,fact", [
    ([5], 1, 5, "bpr_max", "tanh", "linear"), ([16], 9, 0, "top1_max", "tanh", "leaky_relu"),
    ([16], 7, 58, "bpr_max", "relu", "relu"), ([24, 8], 3, 300, "top1_max", "tanh", "linear"),
    ([8], 257, 0, "bpr_max", "tanh", "linear"), ([1], 6, 7, "top1_max", "relu", "relu"),
    ([128], 65, 70, "bpr_max", "tanh", "leaky_relu"), ([8, 8, 8], 64, 64, "top1_max", "relu", "leaky_relu"),
    ([100], 66, 513, "bpr_max", "tanh", "linear")])
def test_step_edges_against_the_restatement(layers, B, n_sample, loss, hact, fact):
    """B = 1 with negatives; n_sample = 0; M = 65, no multiple of 64; M = 303, beyond one pass of the 256-thread row
    loop; B = 257 alone; widths 1 and 128; three layers at M = 128, two whole tiles; M = 303 and 579, three and five
    128-column chunks of the dh_top product; a non-zero state on entry, reg > 0, bpr_reg = 0.7 and (50 items) duplicates throughout"""
    _check_gradients(layers, B, n_sample, loss, hact, fact)


def test_step_from_a_zero_state_and_duplicate_patterns():
    """a zero state; all negatives one item; all of Y one item (every negative equals the positive); reg > 0 throughout"""
    B, n = 17, 20
    _check_gradients([16], B, n, "bpr_max", "tanh", "linear", zero_state=True, seed=6)
    _check_gradients([16], B, n, "top1_max", "tanh", "leaky_relu", Y=np.r_[np.arange(B), np.full(n, 7)], seed=3)
    _check_gradients([8, 8], B, n, "bpr_max", "relu", "relu", X=np.full(B, 5), Y=np.full(B + n, 5), seed=5)


def test_reg_counts_per_slot():
    """an item in k slots of Y — positives and negatives alike — carries k times the regulariser's gradient (the l2
    terms are on the GATHERED rows, all M slots): with the loss's own gradient taken out by difference against reg = 0"""
    B, n, I = 4, 6, 20
    X, Y = np.asarray([3, 3, 4, 5]), np.asarray([9, 1, 2, 9, 9, 9, 11, 12, 1, 13])
    e1 = _check_gradients([8], B, n, "bpr_max", "tanh", "linear", reg=0.5, I=I, X=X, Y=Y, seed=8)
    e0 = _check_gradients([8], B, n, "bpr_max", "tanh", "linear", reg=0.0, I=I, X=X, Y=Y, seed=8)
    dQ = (e1.G["Q"] - e0.G["Q"]).cpu().numpy()
    db = (e1.G["b"] - e0.G["b"]).cpu().numpy()
    V = P.init_tables(I, [8], seed=9)
    assert np.abs(dQ[9] - 4 * 0.5 * V["Q"][9]).max() <= 1e-5 and np.abs(dQ[1] - 2 * 0.5 * V["Q"][1]).max() <= 1e-5
    assert abs(db[9] - 4 * 0.5 * V["b"][9]) <= 1e-5 and abs(db[13] - 0.5 * V["b"][13]) <= 1e-5


# ------------------------------------------------------------------ awkward logits
def _tables_with(I, layers, seed, q_scale, b):
    V = P.init_tables(I, layers, seed=seed)
    V["Q"] = (V["Q"] * q_scale).astype(np.float32)
    V["b"] = np.asarray(b, np.float32)
    return V


@pytest.mark.parametrize("loss", ["bpr_max", "top1_max"])
def test_logits_of_magnitude_80(loss):
    """leaky_relu on logits spread over +-80 (the biases carry them), two of them beyond 88.7, where an unshifted
    float32 exp overflows: the max is subtracted first, the result is finite and within the bar"""
    rs = np.random.RandomState(61)
    I = 40
    V = _tables_with(I, [16], 62, 1.0, rs.uniform(-80, 80, I))
    V["b"][:3] = (95.0, 88.7, -120.0)                       # exp(95) overflows float32
    eng = _check_gradients([16], 12, 30, loss, "tanh", "leaky_relu", I=I, V=V, seed=63)
    assert np.abs(eng.G["b"].cpu().numpy()).max() > 0


def test_all_negatives_below_zero():
    """every logit negative: the row maximum is the masked diagonal's 0, not a negative's value"""
    rs = np.random.RandomState(64)
    I = 40
    V = _tables_with(I, [16], 65, 0.1, -1.0 - 3.0 * rs.rand(I))
    for loss in ("bpr_max", "top1_max"):
        _check_gradients([16], 12, 30, loss, "tanh", "linear", I=I, V=V, seed=66)


@pytest.mark.parametrize("loss", ["bpr_max", "top1_max"])
def test_a_positive_far_above_every_negative(loss):
    """row 0's positive scores +95 and every other score of the row lies near -5: the max runs over the MASKED row (0
    here), so the negatives keep weights of order 1 / M; a max that took the diagonal in would shift them all by 95 and
    leave exp(-100), below float32's normal range"""
    I, B, n = 40, 4, 30
    rs = np.random.RandomState(74)
    b = -5.0 + rs.rand(I)
    b[0] = 95.0
    V = _tables_with(I, [16], 75, 0.1, b)
    Y = np.r_[[0], rs.randint(1, I, size=B - 1 + n)]
    _check_gradients([16], B, n, loss, "tanh", "linear", I=I, V=V, Y=Y, seed=76)


def test_relu_with_every_logit_zero():
    """Q = 0 and b = 0 under relu: every activated logit is 0, every weight 1 / (M - 1), relu'(0) = 0: the loss is
    -log(1/2) (bpr_max) or 1 (top1_max) and no gradient reaches Q, b or the stack"""
    I = 30
    V = _tables_with(I, [8], 67, 0.0, np.zeros(I))
    for loss, want in (("bpr_max", np.log(2.0)), ("top1_max", 1.0)):
        import torch
        eng = _engine(V, [8], 6, 9, loss, "tanh", "relu", reg=0.0)
        rs = np.random.RandomState(68)
        loss2 = torch.zeros(2, device=eng.E_in.device)
        eng.gradients(_i32(eng, rs.randint(I, size=6)), _i32(eng, rs.randint(I, size=15)), loss2)
        assert abs(float(loss2[0]) - want) <= 1e-6 * want and float(loss2[1]) == 0.0
        for name, G in eng.G.items():
            assert not G.any().item(), name


def test_prob_underflows_to_the_floor():
    """bpr_max with every positive 80 below every negative: sigmoid(p - A) ~ 2e-35 and prob = sum s f lies far below
    the 1e-24 inside the log: the row's loss is -log(1e-24) + bpr_reg sum s A^2, finite, and the gradients hold"""
    I, B, n = 40, 8, 24
    b = np.full(I, 40.0)
    b[:B] = -40.0
    V = _tables_with(I, [16], 69, 0.1, b)
    rs = np.random.RandomState(70)
    Y = np.r_[np.arange(B), rs.randint(B, I, size=n)]
    eng = _check_gradients([16], B, n, "bpr_max", "tanh", "linear", reg=0.0, bpr_reg=0.001, I=I, V=V, Y=Y, seed=71)
    assert np.isfinite(eng.G["Q"].cpu().numpy()).all()


# ------------------------------------------------------------------ ids, determinism, empty work, refusals
def test_an_id_outside_the_table_is_dropped():
    """ids -1 and I among the negatives (and one among the inputs): a row of zeros in the forward pass, no gradient row;
    every other gradient as the restatement with an appended zero row has it"""
    I, B, n = 30, 6, 10
    rs = np.random.RandomState(72)
    X, Y = rs.randint(I, size=B), rs.randint(I, size=B + n)
    Y[B + 1], Y[B + 4], X[2] = I, -1, I + 5
    eng = _check_gradients([16], B, n, "bpr_max", "tanh", "linear", I=I, X=X, Y=Y, seed=73)
    touched = np.flatnonzero(eng.G["Q"].cpu().numpy().any(axis=1))
    assert set(touched.tolist()) == set(Y[(Y >= 0) & (Y < I)].tolist())


def test_two_engines_fed_alike_end_byte_identical():
    import torch
    rs = np.random.RandomState(31)
    layers, B, n, I, S = [100], 65, 600, 80, 3
    V = P.init_tables(I, layers, seed=32)
    X, Y = rs.randint(I, size=(S, B)), rs.randint(I, size=(S, B + n))
    reset = (rs.rand(S, B) < 0.2).astype(np.uint8)
    ends = []
    for _ in range(2):
        eng = _engine(V, layers, B, n, "bpr_max", "tanh", "linear", lr=0.01, reg=0.01)
        losses = torch.zeros((S, 2), device=eng.E_in.device)
        eng.run_schedule(X, Y, reset, losses)
        ends.append((eng, losses))
    (a, la), (b, lb) = ends
    assert torch.equal(la, lb) and bool(torch.isfinite(la).all())
    for name in a.tables():
        assert torch.equal(a.tables()[name], b.tables()[name]), name
        assert torch.equal(a.m[name], b.m[name]) and torch.equal(a.v[name], b.v[name]), name
    for x, y in zip(a.states, b.states):
        assert torch.equal(x, y)


def test_empty_work_and_refusals():
    import torch
    layers, I = [8], 20
    V = P.init_tables(I, layers, seed=41)
    eng = _engine(V, layers, 4, 3)
    dev = eng.E_in.device
    before = _tables(eng)
    loss2 = torch.ones(2, device=dev)
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    eng.step(empty, empty, loss2)                                   # B = 0
    assert eng.t == 0 and not loss2.any().item()
    eng.run_schedule(np.zeros((0, 4), np.int32), np.zeros((0, 7), np.int32), np.zeros((0, 4), np.uint8),
                     torch.zeros((0, 2), device=dev))                # S = 0
    assert eng.t == 0
    for name, t in _tables(eng).items():
        assert np.array_equal(t, before[name]), name
    four, five = (torch.zeros(k, dtype=torch.int32, device=dev) for k in (4, 5))
    with pytest.raises(ValueError, match="batch larger than max_batch"):
        eng.step(five, torch.zeros(8, dtype=torch.int32, device=dev), loss2)
    with pytest.raises(ValueError, match=r"Y must hold len\(X\) \+ n_sample items"):
        eng.step(four, four, loss2)
    with pytest.raises(ValueError, match=r"Y \[steps, batch \+ n_sample\]"):
        eng.run_schedule(np.zeros((1, 4), np.int32), np.zeros((1, 4), np.int32), np.zeros((1, 4), np.uint8),
                         torch.zeros((1, 2), device=dev))
    with pytest.raises(ValueError, match=r"Y holds an item outside \[0, 20\)"):
        eng.run_schedule(np.zeros((1, 4), np.int32), np.full((1, 7), I, np.int32), np.zeros((1, 4), np.uint8),
                         torch.zeros((1, 2), device=dev))
    lone = _engine(V, layers, 4, 0)                                  # n_sample = 0: a batch of one has no negative
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(NotImplementedError, match=r"batch \+ n_sample = 1: a row needs at least one negative"):
        lone.step(one, one, loss2)
    assert eng.t == 0 and lone.t == 0


def test_gru4recplus_config_drops_in(tmp_path):
    """NeuRec.properties + conf/GRU4RecPlus.properties (the reference's values: 256 + 2048 columns) on ml-100k with
    by_time=True: one epoch through neurec_amd.main; the metrics header, the two notes and the `epoch` line, in order;
    finite metrics; predict()'s two modes"""
    from neurec_amd.model.sequential_recommender.GRU4RecPlus import DEVIATIONS
    model = _run(tmp_path, ["--recommender=GRU4RecPlus", "--epochs=1"])
    eng = model.engine
    assert type(eng).__name__ == "GRU4RecPlusEngine" and eng.layers == [100] and eng.max_batch == 256
    assert eng.n_sample == 2048 and eng.loss == "bpr_max" and eng.t > 20
    folder = os.path.join(str(tmp_path), "log", "ml-100k", "GRU4RecPlus")
    files = os.listdir(folder)
    assert len(files) == 1
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "GRU4RecPlus's hyperparameters:" in text
    note = "negatives are sampled as ranks"
    lines = [ln for ln in text.splitlines() if re.search(r"metrics:\t|epoch \d+:\t", ln) or DEVIATIONS in ln or note in ln]
    kinds = ["m" if "metrics:" in ln else "d" if DEVIATIONS in ln else "r" if note in ln else "e" for ln in lines]
    assert kinds == ["m", "d", "r", "e"], kinds
    shown = np.asarray([float(x) for x in re.findall(r"epoch 0:\t(.+)", text)[0].split()])
    assert np.all(np.isfinite(shown)) and shown.max() > 0
    for t in eng.tables().values():
        assert bool(t.isfinite().all())
    full = model.predict([0, 5, 9], None)
    assert tuple(full.shape) == (3, model.items_num) and full.is_cuda
    full = full.cpu().numpy()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])


def test_plugin_refusals(tmp_path):
    with pytest.raises(ValueError, match="There is not loss named 'top1'."):
        _run(tmp_path, ["--recommender=GRU4RecPlus", "--epochs=1", "--loss=top1"])
    with pytest.raises(ValueError, match="batch_size=2000 is larger than the 943 users"):
        _run(tmp_path, ["--recommender=GRU4RecPlus", "--epochs=1", "--batch_size=2000"])
    with pytest.raises(NotImplementedError, match="n_sample=9000 is not supported"):
        _run(tmp_path, ["--recommender=GRU4RecPlus", "--epochs=1", "--n_sample=9000"])
