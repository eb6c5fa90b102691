"""GRU4Rec on the GPU (csrc/gru4rec.hip through neurec_amd/gru4rec.py): every step of the reference class's trace with
the fetched states, the users' final states and predict(), the edge shapes of the step on its gradients, state across
steps through run_schedule, the recorded epoch, the sequence kernel's tiles, determinism, empty work, the refusals, the
scoring kernel and the drop-in run through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from neurec_amd import defaults
import gru4rec_restatement as P
from gru4rec_restatement import CASES
from test_gru4rec_cpu import golden_table

pytestmark = pytest.mark.gpu

T = 16                              # NRHIP_GRU4REC_TILE: users per workgroup of the sequence kernel


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_gru4rec")


def _engine(V, layers, max_batch, loss="top1", hact="tanh", fact="linear", lr=0.001, reg=0.0):
    from neurec_amd.gru4rec import GRU4RecEngine
    cells = [tuple(V["%s%d" % (n, l)] for n in ("Wg", "bg", "Wc", "bc")) for l in range(len(layers))]
    return GRU4RecEngine(V["E_in"], V["Q"], V["b"], cells, lr, reg, max_batch, loss=loss, hidden_act=hact,
                         final_act=fact)


def _i32(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(eng.E_in.device)


def _u8(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(eng.E_in.device)


def _tables(eng):
    return {k: t.cpu().numpy() for k, t in eng.tables().items()}


def _set_states(eng, states):
    import torch
    for dst, s in zip(eng.states, states):
        dst[:len(s)] = torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).to(dst.device)


def _close(got, want, bar, what):
    """the project's rule: 4 x the reference's own f32-to-f64 distance plus 1e-5 max|want|; both figures printed"""
    err = np.abs(got.astype(np.float64) - want).max(initial=0)
    print("%s: device err %.3g, reference f32 err %.3g" % (what, err, bar))
    assert got.shape == want.shape and err <= 4 * bar + 1e-5 * np.abs(want).max(initial=0), (what, err, bar)


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Every variable and the fetched states after every step against the f64 trace: within 4x the reference's own
    f32-to-f64 distance of that step and tensor (read from the golden) plus 1e-5 max|want|.  Rows of E_in, Q and b
    outside <case>_rows_* are bit-equal to their initial value; the gradient buffers are zero again afterwards; the
    reset slots' states are zero."""
    import torch
    g = golden
    loss, hact, fact, layers, reg = CASES[case]
    names = P.table_names(len(layers))
    B = int(g["batch_step"])
    eng = _engine({n: g["%s_init_%s" % (case, n)] for n in names}, layers, B, loss, hact, fact, float(g["lr"]), reg)
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


def test_user_states_and_predict_match_the_reference(golden):
    """_get_user_embeddings() and predict(), full and candidate mode, after the trained case, under the trace's rule"""
    import torch
    g = golden
    case = P.PREDICT_CASE
    loss, hact, fact, layers, reg = CASES[case]
    names = P.table_names(len(layers))
    B = int(g["batch_step"])
    eng = _engine({n: g["%s_init_%s" % (case, n)] for n in names}, layers, B, loss, hact, fact, float(g["lr"]), reg)
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
def _check_gradients(layers, B, loss, hact, fact, reg=0.01, I=50, X=None, Y=None, zero_state=False, seed=0):
    """gradients() and the new states against the float64 restatement, 1e-5 max|want| per tensor (fp32 sums of at most
    a few hundred O(1) terms).  Adam is left out on purpose: its first step is lr sign(g) and hides the size of an error"""
    import torch
    rs = np.random.RandomState(seed)
    V = P.init_tables(I, layers, seed=seed + 1)
    eng = _engine(V, layers, B, loss, hact, fact, reg=reg)
    X = rs.randint(I, size=B) if X is None else np.asarray(X)
    Y = rs.randint(I, size=B) if Y is None else np.asarray(Y)
    states = [np.zeros((B, n), np.float32) if zero_state else (0.5 * rs.randn(B, n)).astype(np.float32) for n in layers]
    _set_states(eng, states)
    loss2 = torch.zeros(2, device=eng.E_in.device)
    before = _tables(eng)
    eng.gradients(_i32(eng, X), _i32(eng, Y), loss2)
    V64 = {k: v.astype(np.float64) for k, v in V.items()}
    (lt, lr_), G, hs = P.gradients(V64, X, Y, [s.astype(np.float64) for s in states], loss, hact, fact, reg)
    got2 = loss2.cpu().numpy().astype(np.float64)
    assert abs(got2[0] - lt) <= 1e-5 * abs(lt) and abs(got2[1] - lr_) <= 1e-5 * abs(lr_), (got2, lt, lr_)
    for l in range(len(layers)):
        err = np.abs(eng.h_new[l][:B].cpu().numpy() - hs[l]).max()
        assert err <= 1e-5 * np.abs(hs[l]).max(), ("state", l, err)
        assert np.array_equal(eng.states[l][:B].cpu().numpy(), states[l])          # gradients() moves no state
    for name, want in G.items():
        got = eng.G[name].cpu().numpy()
        err = np.abs(got - want).max()
        assert err <= 1e-5 * np.abs(want).max(), (name, err, np.abs(want).max())
    for name, t in _tables(eng).items():                                           # and no table
        assert np.array_equal(t, before[name]), name
    return eng


@pytest.mark.parametrize("layers,B,loss,hact,fact", [
    ([1], 1, "top1", "tanh", "linear"), ([5], 2, "bpr", "relu", "relu"), ([16], 63, "top1", "tanh", "leaky_relu"),
    ([100], 65, "top1", "tanh", "linear"), ([24, 8], 64, "bpr", "tanh", "leaky_relu"),
    ([8, 8, 8], 65, "top1", "relu", "relu"), ([128], 64, "bpr", "tanh", "linear"), ([5], 1, "bpr", "tanh", "linear")])
def test_step_edges_against_the_restatement(layers, B, loss, hact, fact):
    """every width, depth, batch size, loss and activation of the issue's list, a non-zero state on entry, reg > 0 and
    (50 items) duplicates in X and in Y from B = 63 on"""
    _check_gradients(layers, B, loss, hact, fact)


def test_step_duplicate_patterns():
    """all of Y one item; all of X one item; one item input and output of every slot; a zero state; reg > 0 throughout"""
    B = 17
    _check_gradients([16], B, "top1", "tanh", "linear", Y=np.full(B, 7), seed=3)
    _check_gradients([16], B, "bpr", "tanh", "leaky_relu", X=np.full(B, 9), seed=4)
    _check_gradients([8, 8], B, "top1", "relu", "relu", X=np.full(B, 5), Y=np.full(B, 5), seed=5)
    _check_gradients([16], B, "bpr", "tanh", "linear", zero_state=True, seed=6)


def test_reg_counts_per_slot():
    """an item in k slots carries k times the regulariser's gradient (the l2 terms are on the GATHERED rows): with the
    loss's own gradient taken out by difference against reg = 0"""
    B, I = 8, 20
    X, Y = np.asarray([3, 3, 3, 4, 5, 6, 7, 8]), np.asarray([9, 9, 1, 2, 9, 9, 0, 11])
    e1 = _check_gradients([8], B, "top1", "tanh", "linear", reg=0.5, I=I, X=X, Y=Y, seed=8)
    e0 = _check_gradients([8], B, "top1", "tanh", "linear", reg=0.0, I=I, X=X, Y=Y, seed=8)
    dE = (e1.G["E_in"] - e0.G["E_in"]).cpu().numpy()
    dQ = (e1.G["Q"] - e0.G["Q"]).cpu().numpy()
    V = P.init_tables(I, [8], seed=9)
    assert np.abs(dE[3] - 3 * 0.5 * V["E_in"][3]).max() <= 1e-5 and np.abs(dE[4] - 0.5 * V["E_in"][4]).max() <= 1e-5
    assert np.abs(dQ[9] - 4 * 0.5 * V["Q"][9]).max() <= 1e-5 and np.abs(dQ[1] - 0.5 * V["Q"][1]).max() <= 1e-5


# ------------------------------------------------------------------ state across steps
def _schedule_against_restatement(V, layers, X, Y, reset, loss, hact, fact, reg, lr):
    """the engine through run_schedule and the restatement stepped the same way, in float64 and in float32: states and
    variables within 4 x the float32 restatement's own distance from the float64 one plus 1e-5 max|want|"""
    import torch
    B = X.shape[1]
    eng = _engine(V, layers, B, loss, hact, fact, lr=lr, reg=reg)
    losses = torch.zeros((len(X), 2), device=eng.E_in.device)
    eng.run_schedule(X, Y, reset, losses)
    st64, st32 = (P.State(V, layers, B, lr=lr, dtype=dt) for dt in (np.float64, np.float32))
    for s in range(len(X)):
        for st in (st64, st32):
            P.step(st, X[s], Y[s], loss, hact, fact, reg, reset=reset[s])
    assert eng.t == len(X) and np.isfinite(losses.cpu().numpy()).all()
    for l in range(len(layers)):
        _close(eng.states[l][:B].cpu().numpy(), st64.states[l], np.abs(st32.states[l] - st64.states[l]).max(),
               "state %d after %d steps" % (l, len(X)))
    for name, got in _tables(eng).items():
        _close(got, st64.V[name], np.abs(st32.V[name] - st64.V[name]).max(), "%s after %d steps" % (name, len(X)))
    return eng, st64


def test_state_is_carried_and_reset_across_steps():
    """six steps with a reset mask in the middle: the states reach the next step, the masked slots start from zero"""
    rs = np.random.RandomState(11)
    layers, B, I, S = [24, 8], 12, 40, 6
    V = P.init_tables(I, layers, seed=12)
    X, Y = rs.randint(I, size=(S, B)), rs.randint(I, size=(S, B))
    reset = np.zeros((S, B), np.uint8)
    reset[2, [0, 5, 11]] = 1
    reset[3, [5]] = 1
    eng, st = _schedule_against_restatement(V, layers, X, Y, reset, "bpr", "tanh", "leaky_relu", 0.01, 0.01)
    # the state matters: the same feeds from zero states every step end elsewhere
    fresh = P.State(V, layers, B, lr=0.01)
    for s in range(S):
        P.step(fresh, X[s], Y[s], "bpr", "tanh", "leaky_relu", 0.01, reset=np.ones(B, bool))
    assert np.abs(fresh.V["Wg0"] - st.V["Wg0"]).max() > 1e-4


def test_the_recorded_epoch_ends_at_the_reference_tables(golden):
    """train_model()'s epoch of the golden run through the plugin's schedule and run_schedule: the end tables under the
    trace's rule"""
    import torch
    from neurec_amd.model.sequential_recommender.GRU4Rec import session_parallel_schedule
    g = golden
    loss, hact, fact, layers, reg = CASES[P.PREDICT_CASE]
    names = P.table_names(len(layers))
    B = int(g["batch_epoch"])
    X, Y, reset = session_parallel_schedule(g["offset_idx"], g["epoch_perm"], B, g["data_uit"][:, 1])
    eng = _engine({n: g["epoch_init_" + n] for n in names}, layers, B, loss, hact, fact, float(g["lr"]), reg)
    losses = torch.zeros((len(X), 2), device=eng.E_in.device)
    eng.run_schedule(X, Y, reset, losses)
    assert eng.t == len(g["epoch_X"])
    for name, got in _tables(eng).items():
        w64, w32 = (golden_table(g, "epoch", tag, name, 0) for tag in ("f64", "f32"))
        _close(got, w64, np.abs(w32 - w64).max(), "epoch end %s" % name)


# ------------------------------------------------------------------ the sequence kernel
@pytest.fixture(scope="module")
def sequences():
    """40 users: lengths 0, 1, 2 and 70, then lengths 1 and 40 in turn (users 4..19), then short random ones"""
    rs = np.random.RandomState(21)
    I, layers = 60, [24, 8]
    lens = [0, 1, 2, 70] + [1, 40] * 8 + rs.randint(1, 12, size=20).tolist()
    seq_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seq = rs.randint(I, size=int(seq_ptr[-1])).astype(np.int32)
    V = P.init_tables(I, layers, seed=22)
    eng = _engine(V, layers, 4, hact="tanh")
    eng.set_sequences(seq_ptr, seq)
    n = len(lens)
    h64 = P.user_states(V, layers, "tanh", seq_ptr, seq, range(n))
    h32 = P.user_states(V, layers, "tanh", seq_ptr, seq, range(n), dtype=np.float32)
    return dict(eng=eng, V=V, layers=layers, lens=np.asarray(lens), seq_ptr=seq_ptr, seq=seq, h64=h64, h32=h32)


@pytest.mark.parametrize("users", [[0, 1, 2, 3], list(range(T - 1)), list(range(T)), list(range(T + 1)),
                                   list(range(4, 20)), [3, 3, 7], list(range(40)), [5]],
                         ids=["lengths_0_1_2_70", "T-1", "T", "T+1", "lengths_1_and_40", "listed_twice", "all", "one"])
def test_user_states_against_the_restatement(sequences, users):
    """per user: within 4 x the float32 restatement's own distance from the float64 one at that user's length plus
    1e-5 max|want|; a user without items gets zeros"""
    s = sequences
    H = s["eng"].user_states(users).cpu().numpy()
    assert H.shape == (len(users), s["layers"][-1])
    for row, u in enumerate(users):
        want = s["h64"][u]
        bar = np.abs(s["h32"][u] - want).max()
        err = np.abs(H[row] - want).max()
        if s["lens"][u] in (0, 1, 2, 40, 70):
            print("user %d (length %d): device err %.3g, float32 restatement err %.3g" % (u, s["lens"][u], err, bar))
        assert err <= 4 * bar + 1e-5 * np.abs(want).max(), (u, err, bar)
        if s["lens"][u] == 0:
            assert not H[row].any()
    if users == [3, 3, 7]:
        assert np.array_equal(H[0], H[1])


def test_a_user_s_row_does_not_depend_on_its_tile(sequences):
    """bit-equal alone, in a full tile of neighbours, and among every user"""
    s = sequences
    everyone = s["eng"].user_states().cpu().numpy()
    assert everyone.shape == (40, s["layers"][-1])
    tile = s["eng"].user_states(list(range(4, 20))).cpu().numpy()
    for u in (3, 4, 5, 19):
        alone = s["eng"].user_states([u]).cpu().numpy()[0]
        assert np.array_equal(alone, everyone[u]), u
        if 4 <= u < 20:
            assert np.array_equal(alone, tile[u - 4]), u


def test_user_states_agree_with_the_training_forward_path(sequences):
    """the same items fed one at a time through gradients() (no apply), the new states handed over by advance(): the
    top state after the last item, under the sequence kernel's bound"""
    import torch
    s = sequences
    eng = s["eng"]
    loss2 = torch.zeros(2, device=eng.E_in.device)
    for u in (2, 3):
        eng.reset_states()
        items = s["seq"][s["seq_ptr"][u]:s["seq_ptr"][u + 1]]
        for item in items:
            x = _i32(eng, [item])
            eng.gradients(x, x, loss2)
            eng.advance(1)
        for G in eng.G.values():
            G.zero_()
        got = eng.states[-1][0].cpu().numpy()
        want = s["h64"][u]
        bar = np.abs(s["h32"][u] - want).max()
        err = np.abs(got - want).max()
        print("user %d through the step: err %.3g, float32 restatement err %.3g" % (u, err, bar))
        assert err <= 4 * bar + 1e-5 * np.abs(want).max()
        H = eng.user_states([u]).cpu().numpy()[0]
        assert np.abs(H - got).max() <= 4 * bar + 1e-5 * np.abs(want).max()
    eng.reset_states()


# ------------------------------------------------------------------ other checks
def test_two_engines_fed_alike_end_byte_identical():
    import torch
    rs = np.random.RandomState(31)
    layers, B, I, S = [100], 65, 80, 3
    V = P.init_tables(I, layers, seed=32)
    X, Y = rs.randint(I, size=(S, B)), rs.randint(I, size=(S, B))
    reset = (rs.rand(S, B) < 0.2).astype(np.uint8)
    ends = []
    for _ in range(2):
        eng = _engine(V, layers, B, "top1", "tanh", "linear", lr=0.01, reg=0.01)
        losses = torch.zeros((S, 2), device=eng.E_in.device)
        eng.run_schedule(X, Y, reset, losses)
        ends.append((eng, losses))
    (a, la), (b, lb) = ends
    assert torch.equal(la, lb)
    for name in a.tables():
        assert torch.equal(a.tables()[name], b.tables()[name]), name
        assert torch.equal(a.m[name], b.m[name]) and torch.equal(a.v[name], b.v[name]), name
    for x, y in zip(a.states, b.states):
        assert torch.equal(x, y)


def test_empty_work_is_accepted():
    import torch
    layers, I = [8], 20
    V = P.init_tables(I, layers, seed=41)
    eng = _engine(V, layers, 4)
    before = _tables(eng)
    loss2 = torch.ones(2, device=eng.E_in.device)
    empty = torch.zeros(0, dtype=torch.int32, device=eng.E_in.device)
    eng.step(empty, empty, loss2)                                   # B = 0
    assert eng.t == 0 and not loss2.any().item()
    eng.run_schedule(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32), np.zeros((0, 4), np.uint8),
                     torch.zeros((0, 2), device=eng.E_in.device))    # S = 0
    assert eng.t == 0
    eng.set_sequences(np.asarray([0, 2, 2]), np.asarray([1, 3]))
    H = eng.user_states([])                                          # an empty user list
    assert tuple(H.shape) == (0, 8)
    assert tuple(eng.score([]).shape) == (0, I)
    for name, t in _tables(eng).items():
        assert np.array_equal(t, before[name]), name
    with pytest.raises(ValueError, match="batch larger than max_batch"):
        five = torch.zeros(5, dtype=torch.int32, device=eng.E_in.device)
        eng.step(five, five, loss2)


def test_a_schedule_with_an_item_outside_the_table_is_refused():
    import torch
    layers, I = [8], 20
    eng = _engine(P.init_tables(I, layers, seed=43), layers, 4)
    ok, zero = np.zeros((1, 4), np.int32), np.zeros((1, 4), np.uint8)
    losses = torch.zeros((1, 2), device=eng.E_in.device)
    for bad in (-1, I):
        with pytest.raises(ValueError, match=r"X holds an item outside \[0, 20\)"):
            eng.run_schedule(np.full((1, 4), bad, np.int32), ok, zero, losses)
        with pytest.raises(ValueError, match=r"Y holds an item outside \[0, 20\)"):
            eng.run_schedule(ok, np.full((1, 4), bad, np.int32), zero, losses)
    assert eng.t == 0


@pytest.mark.parametrize("fact", ["relu", "leaky_relu", "linear"])
def test_score_is_the_activated_product(fact):
    """score() against act(H Q^T + b) on the host in float64 (1e-5 max|want|: a 40-term fp32 dot product); widths and
    counts that are no multiple of the 64 x 64 tile; for linear, eval_factors() reproduces score()"""
    layers, I = [40], 131
    V = P.init_tables(I, layers, seed=51)
    eng = _engine(V, layers, 4, fact=fact)
    lens = np.asarray([3, 0, 5, 1, 2] * 14)                          # 70 users
    rs = np.random.RandomState(52)
    seq_ptr = np.concatenate([[0], np.cumsum(lens)])
    eng.set_sequences(seq_ptr, rs.randint(I, size=int(seq_ptr[-1])))
    H = eng.user_states().cpu().numpy().astype(np.float64)
    users = np.arange(70)[::-1].copy()
    got = eng.score(users).cpu().numpy()
    want = P.predict(H[users], V["Q"].astype(np.float64), V["b"].astype(np.float64), fact)
    assert got.shape == (70, I) and got.dtype == np.float32
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    if fact != "linear":
        assert (got >= 0).all() if fact == "relu" else (got < 0).any()
        assert eng.eval_factors() is None
    else:
        Pu, Qi = eng.eval_factors()
        assert tuple(Pu.shape) == (70, 41) and tuple(Qi.shape) == (I, 41)
        prod = (Pu.cpu().numpy().astype(np.float64) @ Qi.cpu().numpy().astype(np.float64).T)[users]
        assert np.abs(got - prod).max() <= 1e-5 * np.abs(prod).max()


def _run(tmp_path, argv):
    import importlib.util
    from neurec_amd.main import main
    spec = importlib.util.spec_from_file_location(
        "make_ml100k_rating_fixture", os.path.join(os.path.dirname(__file__), "golden", "make_ml100k_rating_fixture.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    data_dir = os.path.join(str(tmp_path), "dataset")
    os.makedirs(data_dir, exist_ok=True)
    if not os.path.isfile(os.path.join(data_dir, "ml-100k.rating")):
        mk.write_rating_file(os.path.join(data_dir, "ml-100k.rating"))
    path = defaults.write_default_configs(str(tmp_path), overrides={
        "data.input.path": data_dir, "data.cache.path": str(tmp_path), "by_time": "True", "topk": "[10, 20]"})
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        return main(argv=argv, properties=path)
    finally:
        os.chdir(cwd)


def test_gru4rec_config_drops_in(tmp_path):
    """NeuRec.properties + conf/GRU4Rec.properties (the reference's values) on ml-100k with by_time=True: two epochs
    through neurec_amd.main; the metrics header, the deviation line and two `epoch` lines, in order, no loss line; the
    evaluator's metrics are identical on the factor path and on the score-matrix path; predict()'s two modes"""
    from neurec_amd.model.sequential_recommender.GRU4Rec import DEVIATIONS
    model = _run(tmp_path, ["--recommender=GRU4Rec", "--epochs=2"])
    assert model.engine.layers == [100] and model.engine.max_batch == 256 and model.engine.t > 100
    folder = os.path.join(str(tmp_path), "log", "ml-100k", "GRU4Rec")
    files = os.listdir(folder)
    assert len(files) == 1
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "GRU4Rec's hyperparameters:" in text and "loss" not in text.split("metrics:")[-1].lower()
    lines = [ln for ln in text.splitlines() if re.search(r"metrics:\t|epoch \d+:\t", ln) or DEVIATIONS in ln]
    kinds = ["m" if "metrics:" in ln else "d" if DEVIATIONS in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)
             for ln in lines]
    assert kinds == ["m", "d", "e0", "e1"], kinds
    shown = np.asarray([float(x) for x in re.findall(r"epoch 1:\t(.+)", text)[0].split()])
    assert np.all(np.isfinite(shown)) and shown.max() > 0
    by_factors = model.evaluator.evaluate(model)
    assert model.get_eval_factors() is not None
    model.get_eval_factors = lambda: None
    by_scores = model.evaluator.evaluate(model)
    del model.get_eval_factors
    assert by_factors == by_scores, (by_factors, by_scores)
    full = model.predict([0, 5, 9], None)
    assert tuple(full.shape) == (3, model.items_num) and full.is_cuda
    full = full.cpu().numpy()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])
    assert np.array_equal(cand[1], full[1][[7]])


def test_plugin_refusals(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="There is not final_act named 'softmax'."):
        _run(tmp_path, ["--recommender=GRU4Rec", "--epochs=1", "--final_act=softmax"])
    with pytest.raises(ValueError, match="batch_size=2000 is larger than the 943 users"):
        _run(tmp_path, ["--recommender=GRU4Rec", "--epochs=1", "--batch_size=2000"])
    with pytest.raises(NotImplementedError, match="layer width 129 is not supported"):
        _run(tmp_path, ["--recommender=GRU4Rec", "--epochs=1", "--layers=[129]"])
    from neurec_amd import parallel
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)                                # WORLD_SIZE > 1
    with pytest.raises(NotImplementedError, match="one GPU"):
        _run(tmp_path, ["--recommender=GRU4Rec", "--epochs=1"])
