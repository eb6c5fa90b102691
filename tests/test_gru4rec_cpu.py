"""GRU4Rec without a GPU: the float64 restatement the GPU tests lean on (tests/gru4rec_restatement.py) against the
reference class's own trace, the plugin's session-parallel schedule against the recorded epoch and against the
reference loop on hand-made length lists, `_init_data`, the header / binding, the defaults row, the refusal texts and
`recommender=GRU4Rec`."""
import configparser
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_golden
import gru4rec_restatement as P
from gru4rec_restatement import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_gru4rec")


def golden_table(g, case, tag, name, step):
    """variable `name` of the trace after `step` (0-based), full size, as float64"""
    t = g["%s_init_%s" % (case, name)].astype(np.float64)
    delta = g["%s_%s_%s" % (case, tag, name)][step]
    if name in ("E_in", "Q", "b"):
        rows = g["%s_rows_%s" % (case, name)]
        t[rows] = t[rows] + delta
        return t
    return t + delta


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_restatement_equals_the_f64_trace(golden, case):
    """every variable and every fetched state after each of the three steps: 1e-12, the bar the FPMCplus restatement
    met"""
    g = golden
    loss, hact, fact, layers, reg = CASES[case]
    names = P.table_names(len(layers))
    st = P.State({n: g["%s_init_%s" % (case, n)] for n in names}, layers, int(g["batch_step"]), lr=float(g["lr"]))
    X, Y, reset = g[case + "_X"], g[case + "_Y"], g[case + "_reset"]
    assert len(set(X[0].tolist())) < len(X[0]) and len(set(Y[0].tolist())) < len(Y[0])       # duplicates
    assert set(X[0].tolist()) & set(Y[0].tolist())                                            # input and output at once
    for s in range(len(X)):
        _, _, hs = P.gradients(st.V, X[s], Y[s], st.states, loss, hact, fact, reg)
        P.step(st, X[s], Y[s], loss, hact, fact, reg, reset=reset[s])
        for l in range(len(layers)):
            assert np.abs(hs[l] - g["%s_f64_state%d" % (case, l)][s]).max() <= 1e-12, (case, s, l)
            assert not st.states[l][reset[s]].any()
        for n in names:
            assert np.abs(st.V[n] - golden_table(g, case, "f64", n, s)).max() <= 1e-12, (case, s, n)


def test_the_restatement_gives_the_reference_user_states_and_predict(golden):
    """The reference keeps the user vectors in a float32 array (GRU4Rec.py:183) and casts predict()'s result to float32
    (GRU4Rec.py:246) whatever the graph's width, so its float64 run holds float32-rounded values here: the restatement
    must lie within half a float32 ulp (2^-24 relative) of them, element by element — the rounding itself and no more.
    predict() is restated from the reference's own rounded user vectors, so that only its own cast is in the bound."""
    g = golden
    case = P.PREDICT_CASE
    loss, hact, fact, layers, reg = CASES[case]
    names = P.table_names(len(layers))
    V = {n: golden_table(g, case, "f64", n, len(g[case + "_X"]) - 1) for n in names}
    U = int(g["shape"][0])
    half_ulp = 2.0 ** -24
    H = P.user_states(V, layers, hact, g["seq_ptr"], g["seq"], range(U))
    want = g["user_emb_f64"]
    assert np.array_equal(want, want.astype(np.float32).astype(np.float64))           # float32 values in a float64 array
    assert (np.abs(H - want) <= half_ulp * np.abs(want) + 1e-12 * half_ulp).all()
    users = g["predict_users"]
    full = P.predict(want[users], V["Q"], V["b"], fact)
    assert (np.abs(full - g["predict_f64"]) <= half_ulp * np.abs(g["predict_f64"]) + 1e-12 * half_ulp).all()
    cand = np.stack([full[k][c] for k, c in enumerate(g["predict_cand"])])
    assert (np.abs(cand - g["predict_cand_f64"]) <= half_ulp * np.abs(g["predict_cand_f64"]) + 1e-12 * half_ulp).all()


def test_the_gradients_equal_autograd():
    """the hand-written backward pass against torch autograd in float64, every loss and activation, a non-zero state"""
    import torch
    rs = np.random.RandomState(5)
    for loss in ("top1", "bpr"):
        for hact, fact, layers in (("tanh", "linear", [5]), ("relu", "leaky_relu", [6, 3]), ("tanh", "relu", [3, 3, 3])):
            I, B = 17, 9
            V = {k: v.astype(np.float64) for k, v in P.init_tables(I, layers, seed=3).items()}
            X, Y = rs.randint(I, size=B), rs.randint(I, size=B)
            X[1], Y[2] = X[0], Y[0]
            states = [0.3 * rs.randn(B, n) for n in layers]
            (lt, lr_), G, _ = P.gradients(V, X, Y, states, loss, hact, fact, 0.05)
            T = {k: torch.tensor(v, requires_grad=True) for k, v in V.items()}
            x = T["E_in"][torch.as_tensor(X)]
            x0 = x
            for l, s in enumerate(states):
                s = torch.tensor(s)
                n = s.shape[1]
                gts = torch.sigmoid(torch.cat([x, s], 1) @ T["Wg%d" % l] + T["bg%d" % l])
                r, u = gts[:, :n], gts[:, n:]
                pre = torch.cat([x, r * s], 1) @ T["Wc%d" % l] + T["bc%d" % l]
                c = torch.relu(pre) if hact == "relu" else torch.tanh(pre)
                x = u * s + (1 - u) * c
            Qy, by = T["Q"][torch.as_tensor(Y)], T["b"][torch.as_tensor(Y)]
            Z = x @ Qy.T + by
            A = {"linear": Z, "relu": torch.relu(Z), "leaky_relu": torch.nn.functional.leaky_relu(Z, 0.2)}[fact]
            p = torch.diagonal(A).reshape(-1, 1)
            if loss == "bpr":
                total = (-torch.nn.functional.logsigmoid(p - A)).mean()
            else:
                total = (torch.sigmoid(A - p).mean(1) + torch.sigmoid(A ** 2).mean(1)
                         - torch.sigmoid(p ** 2).squeeze() / B).mean()
            regl = 0.05 * 0.5 * ((x0 ** 2).sum() + (Qy ** 2).sum() + (by ** 2).sum())
            assert abs(float(total.detach()) - lt) <= 1e-12 and abs(float(regl.detach()) - lr_) <= 1e-12
            (total + regl).backward()
            for k in V:
                assert np.abs(T[k].grad.numpy() - G[k]).max() <= 1e-12, (loss, hact, fact, k)


def test_the_makers_shim_ops():
    """tests/golden/make_golden_gru4rec.py attaches reshape, matrix_diag_part, gather (the shim's gather kind),
    random.truncated_normal and the three rnn_cell classes to the shim and checks each on a small hand-computed value —
    the restated GRUCell on x = 1, s = 0.5 and weights 0.5; the shim is put back as it was"""
    from oracle import tf_shim
    spec = importlib.util.spec_from_file_location(
        "make_golden_gru4rec", os.path.join(ROOT, "tests", "golden", "make_golden_gru4rec.py"))
    path = list(sys.path)
    names = ("reshape", "matrix_diag_part", "gather", "random")
    before = {k: getattr(tf_shim, k, None) for k in names}
    had_cells = hasattr(tf_shim.nn, "rnn_cell")
    try:
        maker = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(maker)
        assert maker.attach_ops() is True
        assert all(hasattr(tf_shim, k) for k in names) and hasattr(tf_shim.nn, "rnn_cell")
        assert sorted(maker.P.CASES) == sorted(CASES)
    finally:
        for k, v in before.items():
            if v is None:
                if hasattr(tf_shim, k):
                    delattr(tf_shim, k)
            else:
                setattr(tf_shim, k, v)
        if not had_cells and hasattr(tf_shim.nn, "rnn_cell"):
            del tf_shim.nn.rnn_cell
        tf_shim.set_float("float32")
        sys.path[:] = path


# ------------------------------------------------------------------ the schedule
def _schedule(offset_idx, user_idx, B, items):
    from neurec_amd.model.sequential_recommender.GRU4Rec import session_parallel_schedule
    return session_parallel_schedule(offset_idx, user_idx, B, items)


def _check_against_loop(lengths, perm, B):
    """the plugin's schedule against the reference loop (gru4rec_restatement.epoch_feeds): feeds, zero rows, steps"""
    offset = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    items = (np.arange(offset[-1]) * 7 + 3).astype(np.int32)            # every event its own item
    want = list(P.epoch_feeds(offset, items, np.asarray(perm), B))
    X, Y, reset = _schedule(offset, np.asarray(perm), B, items)
    assert X.shape == Y.shape == reset.shape == (len(want), B) and X.dtype == np.int32 and reset.dtype == np.uint8
    for s, (x, y, zero) in enumerate(want):
        assert np.array_equal(X[s], x) and np.array_equal(Y[s], y), s
        assert np.array_equal(zero, np.ones(B, bool) if s == 0 else reset[s - 1].astype(bool)), s
    return len(want)


def test_the_schedule_equals_the_recorded_epoch(golden):
    g = golden
    X, Y, reset = _schedule(g["offset_idx"], g["epoch_perm"], int(g["batch_epoch"]), g["data_uit"][:, 1])
    assert len(X) == len(g["epoch_X"]) > 20
    assert np.array_equal(X, g["epoch_X"]) and np.array_equal(Y, g["epoch_Y"])
    assert g["epoch_zero"][0].all()
    assert np.array_equal(reset[:-1].astype(bool), g["epoch_zero"][1:])
    np.random.seed(int(g["epoch_seed"]))                                   # the permutation is the global stream's
    assert np.array_equal(np.random.permutation(len(g["offset_idx"]) - 1), g["epoch_perm"])
    # positions instead of items when no item list is given
    Xp, Yp, _ = _schedule(g["offset_idx"], g["epoch_perm"], int(g["batch_epoch"]), None)
    assert np.array_equal(Yp, Xp + 1) and np.array_equal(g["data_uit"][:, 1][Xp], X)


def test_the_schedule_on_hand_made_lengths():
    rs = np.random.RandomState(1)
    assert _check_against_loop([1] * 9, rs.permutation(9), 4) == 0              # all lengths 1: rounds that run no step
    assert _check_against_loop([2, 3, 40, 2, 2, 3, 2, 2, 4, 2], np.arange(10), 3) > 0      # one long user among short
    assert _check_against_loop([5, 3, 4, 6], [2, 0, 3, 1], 4) == 2              # as many users as slots
    n = _check_against_loop([3, 9, 9, 2, 2], np.arange(5), 3)                  # the early end: long sessions abandoned
    assert 0 < n < 8                                                           # the two long users alone hold 16 steps
    for seed in range(20):
        rs = np.random.RandomState(seed)
        n = rs.randint(3, 30)
        _check_against_loop(rs.randint(1, 12, size=n), rs.permutation(n), rs.randint(1, n + 1))


def test_the_schedule_refuses_more_slots_than_users():
    with pytest.raises(ValueError, match="batch_size=5 is larger than the 4 users"):
        _schedule(np.asarray([0, 2, 4, 6, 8]), np.arange(4), 5, None)


# ------------------------------------------------------------------ the plugin on the host
class _Dataset:
    def __init__(self, g):
        U, I = (int(x) for x in g["shape"])
        self.train_matrix = sp.csr_matrix((np.ones(len(g["indices"]), np.float32), g["indices"], g["indptr"]),
                                          shape=(U, I))
        ptr, seq = g["seq_ptr"], g["seq"]
        rows = np.repeat(np.arange(U), np.diff(ptr))
        times = np.concatenate([np.arange(1, n + 1) for n in np.diff(ptr)]).astype(np.float64)
        self.time_matrix = sp.csr_matrix((times, (rows, seq)), shape=(U, I))
        self.num_users, self.num_items = U, I


def _plugin(g, **conf):
    from neurec_amd.model.sequential_recommender.GRU4Rec import GRU4Rec
    base = dict(lr=0.001, reg=0.0, layers=[16], batch_size=16, loss="top1", hidden_act="tanh", final_act="linear",
                epochs=1)
    base.update(conf)
    model = GRU4Rec.__new__(GRU4Rec)                       # the base class wants an evaluator; only the data is at stake
    model.dataset = _Dataset(g)
    return model, base


def test_init_data_equals_the_reference(golden):
    model, _ = _plugin(golden)
    data_uit, offset_idx = model._init_data()
    assert data_uit.dtype == np.int32 and offset_idx.dtype == np.int32
    assert np.array_equal(data_uit, golden["data_uit"]) and np.array_equal(offset_idx, golden["offset_idx"])


def test_find_recommender_resolves_gru4rec():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import SeqAbstractRecommender
    cls = find_recommender("GRU4Rec")
    assert cls.__name__ == "GRU4Rec" and cls.__module__ == "neurec_amd.model.sequential_recommender.GRU4Rec"
    assert issubclass(cls, SeqAbstractRecommender)


def test_defaults_are_written_for_gru4rec(tmp_path):
    """defaults.MODELS["GRU4Rec"] holds the values of the reference's conf/GRU4Rec.properties, written as an ini file
    that the Configurator reads back"""
    from neurec_amd import defaults
    path = defaults.write_default_configs(str(tmp_path))
    parser = configparser.ConfigParser()
    parser.optionxform = str
    parser.read(os.path.join(str(tmp_path), "conf", "GRU4Rec.properties"))
    want = {"lr": "0.0001", "reg": "0.0", "layers": "[100]", "batch_size": "256", "loss": "top1", "hidden_act": "tanh",
            "final_act": "linear", "epochs": "1000"}
    assert dict(parser["hyperparameters"]) == want
    from neurec_amd.util.configurator import Configurator
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=GRU4Rec"])
    finally:
        os.chdir(cwd)
    assert conf["recommender"] == "GRU4Rec"
    assert conf["layers"] == [100] and conf["batch_size"] == 256 and conf["lr"] == 0.0001 and conf["loss"] == "top1"


@pytest.mark.parametrize("key,text", [("hidden_act", "There is not hidden_act named 'gelu'."),
                                      ("final_act", "There is not final_act named 'gelu'."),
                                      ("loss", "There is not loss named 'gelu'.")])
def test_the_refusal_texts_are_the_reference_s(key, text):
    """GRU4Rec.py:34,44,51, from the engine's constructor — before anything touches a GPU"""
    from neurec_amd.gru4rec import GRU4RecEngine
    tabs = P.init_tables(7, [4], seed=1)
    cells = [(tabs["Wg0"], tabs["bg0"], tabs["Wc0"], tabs["bc0"])]
    with pytest.raises(ValueError, match=re.escape(text)):
        GRU4RecEngine(tabs["E_in"], tabs["Q"], tabs["b"], cells, 0.001, 0.0, 8, **{key: "gelu"})


def test_the_engine_refuses_shapes_by_name():
    """layer count, widths and max_batch: refused before a device is asked for, never clamped"""
    from neurec_amd.gru4rec import GRU4RecEngine

    def make(layers, max_batch=8):
        tabs = P.init_tables(7, layers, seed=1)
        cells = [tuple(tabs["%s%d" % (n, l)] for n in ("Wg", "bg", "Wc", "bc")) for l in range(len(layers))]
        return GRU4RecEngine(tabs["E_in"], tabs["Q"], tabs["b"], cells, 0.001, 0.0, max_batch)
    with pytest.raises(NotImplementedError, match="4 layers are not supported"):
        make([4, 4, 4, 4])
    with pytest.raises(NotImplementedError, match="layer width 129 is not supported"):
        make([129])
    with pytest.raises(NotImplementedError, match="max_batch=4097 is not supported"):
        make([4], max_batch=4097)
    with pytest.raises(ValueError, match="max_batch must be at least 1"):
        make([4], max_batch=0)


def test_the_header_declares_the_entries_and_lib_binds_them():
    from neurec_amd import _lib
    with open(os.path.join(ROOT, "include", "neurec_hip.h")) as f:
        text = f.read()
    for name in ("nrhip_gru4rec_step", "nrhip_gru4rec_advance", "nrhip_gru4rec_user_states", "nrhip_gru4rec_scores",
                 "nrhip_gru4rec_workspace_floats"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SIGNATURES
    for name in ("nrhip_gru4rec_advance", "nrhip_gru4rec_user_states", "nrhip_gru4rec_scores"):
        above = re.findall(r"^/\*.*?\*/", text[:text.index("int %s(" % name)], re.S | re.M)[-1]
        assert re.search(r"[Rr]eplaces", above) and "GRU4Rec.py:" in above, name          # cites what it replaces
    assert re.search(r"#define NRHIP_ABI_VERSION 4\b", text)
    from neurec_amd.gru4rec import MAX_BATCH, MAX_LAYERS, MAX_WIDTH, TILE
    for macro, value in (("MAX_LAYERS", MAX_LAYERS), ("MAX_WIDTH", MAX_WIDTH), ("MAX_BATCH", MAX_BATCH), ("TILE", TILE)):
        assert re.search(r"#define NRHIP_GRU4REC_%s %d\b" % (macro, value), text), macro
    block = text[text.index("typedef struct nrhip_gru4rec_step_args"):text.index("} nrhip_gru4rec_step_args;")]
    names = re.findall(r"(?:\*\s*d_|\bnrhip_gru4rec_weights )(\w+)(?:\[\w+\])?;", block)
    fields = [n for n, _ in _lib.Gru4recStepArgs._fields_]
    assert fields[:len(names)] == names
    assert fields[len(names):] == ["n_items", "batch", "final_act", "loss_kind", "reg"]


def test_the_c_entries_refuse_by_name():
    """the bounds of the C entries (host code of the library: no GPU needed, nothing is launched)"""
    from neurec_amd import _lib
    a = _lib.Gru4recStepArgs()
    a.w.n_layers = 4
    with pytest.raises(NotImplementedError, match=r"4 layers outside 1\.\.3"):
        _lib.call("nrhip_gru4rec_step", C.byref(a), None)
    a.w.n_layers, a.w.width[0] = 1, 129
    with pytest.raises(NotImplementedError, match=r"layer width 129 outside 1\.\.128"):
        _lib.call("nrhip_gru4rec_step", C.byref(a), None)
    buf = (C.c_float * 4)()
    a.w.width[0] = 4
    for arr in (a.w.Wg, a.w.bg, a.w.Wc, a.w.bc):
        arr[0] = C.addressof(buf)
    a.batch = 4097
    with pytest.raises(NotImplementedError, match=r"batch 4097 outside 0\.\.4096"):
        _lib.call("nrhip_gru4rec_step", C.byref(a), None)
    a.batch, a.final_act = 0, 5
    with pytest.raises(ValueError, match="unknown final_act 5"):
        _lib.call("nrhip_gru4rec_step", C.byref(a), None)
    a.final_act, a.loss_kind = 0, 3
    with pytest.raises(ValueError, match="unknown loss 3"):
        _lib.call("nrhip_gru4rec_step", C.byref(a), None)
    a.loss_kind = 0
    _lib.call("nrhip_gru4rec_step", C.byref(a), None)                 # batch == 0: no launch, no further pointer
    _lib.call("nrhip_gru4rec_user_states", None, None, 5, 6, None, None, 0, None, C.byref(a.w), None, 4, None)
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.call("nrhip_gru4rec_user_states", None, None, 5, 6, None, None, 0, None, C.byref(a.w), None, 3, None)
    with pytest.raises(NotImplementedError, match=r"width 129 outside 1\.\.128"):
        _lib.call("nrhip_gru4rec_scores", None, 129, None, None, 0, 6, 129, 0, None, 6, None)
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.call("nrhip_gru4rec_scores", None, 4, None, None, 3, 6, 4, 0, None, 5, None)         # ld < n_items
    _lib.call("nrhip_gru4rec_scores", None, 4, None, None, 0, 6, 4, 2, None, 6, None)
    widths = (C.c_int * 1)(4)
    _lib.call("nrhip_gru4rec_advance", None, None, widths, 1, 0, None, None)
    floats = C.c_size_t(0)
    _lib.call("nrhip_gru4rec_workspace_floats", 1, widths, 8, C.byref(floats))
    assert floats.value >= 8 * 8 * 2 + 8 * 4 * 8
