"""SRGNN on the host: the restatement's graph build against the feeds the reference class built, the restatement against
the reference's float64 trace and against central differences, the epoch order and the learning-rate schedule against
the recorded epoch, the plugin's keys and defaults, the initial values, the maker's shim ops, and the refusals that need
no device."""
import configparser
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import srgnn_restatement as P
from srgnn_restatement import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I_TOY = 131


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_srgnn")


def case_init(g, case):
    d = CASES["hybrid" if case == "epoch" else case][0]
    return P.init_tables(I_TOY, d, seed=int(g[case + "_init_seed"]))


def golden_table(g, case, name, s, init=None):
    """the variable after step s of the float64 trace: the initial value plus the stored difference (float32 for the
    vectors, int16 counts of the step's scale for the matrices)"""
    init = case_init(g, case) if init is None else init
    key = "%s_f64_%s" % (case, name)
    if key in g:
        return init[name].astype(np.float64) + g[key][s].astype(np.float64)
    return init[name].astype(np.float64) + g["%s_q_%s" % (case, name)][s].astype(np.float64) * \
        float(g["%s_scale_%s" % (case, name)][s])


def _lost(g, case, name, s):
    """what the storage may have lost of that table: 2^-24 of a float32 difference, half a count of an int16 one"""
    key = "%s_f64_%s" % (case, name)
    if key in g:
        return 2.0 ** -24 * float(np.abs(g[key][s]).max())
    return 0.5 * float(g["%s_scale_%s" % (case, name)][s]) * bool(g["%s_q_%s" % (case, name)][s].any())


def _user_dict(g, ptr="seq_ptr", seq="seq"):
    p, q = g[ptr], g[seq]
    return {u: [int(x) for x in q[p[u]:p[u + 1]]] for u in range(len(p) - 1) if p[u + 1] > p[u]}


# ------------------------------------------------------------------ the cases and the graph build
def test_the_cases_cover_the_issue_s_list(golden):
    g = golden
    assert sorted(CASES) == ["gated", "hybrid", "repeats"] and int(g["batch_step"]) == 20
    assert CASES["hybrid"][:5] == (16, 1, False, 1e-5, 6) and CASES["gated"][:4] == (20, 2, True, 0.0)
    assert CASES["repeats"][:5] == (72, 3, False, 1e-5, 12)
    for case in CASES:
        assert g[case + "_seq"].shape == (4, 20, CASES[case][4]) and g[case + "_target"].shape == (4, 20)
    lrs = g["hybrid_lrs"]
    assert lrs[0] == lrs[1] == np.float32(0.001) and lrs[2] == lrs[3] and abs(lrs[2] - 1e-4) < 1e-10   # drops before step 3
    assert not g["gated_q_B"].any()                                                    # nonhybrid at L2 = 0: B stays put
    for s in range(4):                                       # every batch of `repeats` holds the five named patterns
        rows = [P.session_of(r, I_TOY) for r in g["repeats_seq"][s]]
        assert any(len(set(q)) > 1 and any(a == b for a, b in zip(q, q[1:])) for q in rows)
        assert any(len(set(zip(q, q[1:]))) < len(q) - 1 and len(set(q)) > 1 for q in rows)
        assert any(len(q) == 1 for q in rows) and any(len(q) > 1 and len(set(q)) == 1 for q in rows)
        assert any(len(q) == 12 for q in rows)
    assert len(g["predict_users"]) % 20 and len(g["epoch_order"]) > 10


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_graph_build_equals_the_feed_the_class_built(golden, case):
    """nodes, alias map and both normalised adjacency matrices of every session of every golden step, exactly, after
    dropping the pad nodes the class appends (no edges, mask 0)"""
    g = golden
    for s in range(4):
        adj_in, adj_out = g["%s_%d_adj_in" % (case, s)], g["%s_%d_adj_out" % (case, s)]
        alias, items, mask = (g["%s_%d_%s" % (case, s, k)] for k in ("alias", "items", "mask"))
        for b, row in enumerate(g[case + "_seq"][s]):
            q = P.session_of(row, I_TOY)
            nodes, al, a_in, a_out = P.build_graph(q, np.float64)
            n = len(nodes)
            assert mask[b].sum() == len(q) and mask[b][:len(q)].all()
            assert items[b][:n].tolist() == nodes and (items[b][n:] == I_TOY).all()
            assert alias[b][:len(q)].tolist() == al
            want_in = adj_in[b].astype(np.float32).astype(np.float64)       # the placeholder is float32
            want_out = adj_out[b].astype(np.float32).astype(np.float64)
            assert np.array_equal(want_in[:n, :n], a_in) and np.array_equal(want_out[:n, :n], a_out)
            assert not want_in[n:].any() and not want_in[:, n:].any() and not want_out[n:].any() \
                and not want_out[:, n:].any()


def test_the_graph_build_on_hand_made_sessions():
    """[1, 2, 1, 2, 3]: nodes 1 2 3; edges 1->2 (taken twice, stays 1), 2->1, 2->3.  colsum = (1, 1, 1), rowsum =
    (1, 2, 0 -> 1).  A_in = adj / colsum_j; A_out[i][j] = adj[j][i] / rowsum_j — both divisors by the column index"""
    nodes, alias, a_in, a_out = P.build_graph([1, 2, 1, 2, 3])
    assert nodes == [1, 2, 3] and alias == [0, 1, 0, 1, 2]
    assert a_in.tolist() == [[0, 1, 0], [1, 0, 1], [0, 0, 0]]
    assert a_out.tolist() == [[0, 0.5, 0], [1, 0, 0], [0, 0.5, 0]]
    nodes, alias, a_in, a_out = P.build_graph([6, 6, 6])                     # a self-loop
    assert nodes == [6] and alias == [0, 0, 0] and a_in.tolist() == [[1]] and a_out.tolist() == [[1]]
    nodes, alias, a_in, a_out = P.build_graph([9])
    assert nodes == [9] and not a_in.any() and not a_out.any()


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_restatement_equals_the_f64_trace(golden, case):
    """every variable and the loss after every step in float64: equal up to what the golden's int16 storage lost, plus
    1e-9: Adam's first steps move an entry by lr g / (|g| + 1e-8), so where g is near zero a difference of 1e-16 in g
    between two summation orders shows as up to lr / 1e-8 times as much in the table"""
    g = golden
    d, step, nonhybrid, l2, L, _ = CASES[case]
    init = case_init(g, case)
    feeds = [(g[case + "_seq"][s], g[case + "_target"][s]) for s in range(4)]
    losses, trace = P.train(init, feeds, step, l2, g[case + "_lrs"], nonhybrid, np.float64)
    for s in range(4):
        assert abs(losses[s] - g[case + "_loss_f64"][s]) <= 1e-9 * abs(g[case + "_loss_f64"][s]), (s, losses[s])
        for name in P.NAMES:
            err = np.abs(trace[s][name] - golden_table(g, case, name, s, init)).max()
            assert err <= _lost(g, case, name, s) + 1e-9, (case, s, name, err)


def test_the_float32_restatement_stays_within_the_rule_of_the_trace(golden):
    """the float32 twin of the restatement under the rule the device is held to"""
    g = golden
    for case in sorted(CASES):
        d, step, nonhybrid, l2, L, _ = CASES[case]
        init = case_init(g, case)
        feeds = [(g[case + "_seq"][s], g[case + "_target"][s]) for s in range(4)]
        losses, trace = P.train(init, feeds, step, l2, g[case + "_lrs"], nonhybrid, np.float32)
        for s in range(4):
            for name in P.NAMES:
                want = golden_table(g, case, name, s, init)
                err = np.abs(trace[s][name].astype(np.float64) - want).max()
                assert err <= 4 * float(g["%s_gap_%s" % (case, name)][s]) + 1e-5 * np.abs(want).max(), (case, s, name)


def test_the_gradients_equal_central_differences_on_the_repeats_shapes(golden):
    """the hand-written backward pass in float64 against (f(v + h) - f(v - h)) / 2h on entries of all 14 variables, on a
    batch of `repeats` (hidden_size 72, three iterations: the state's four gradient terms are all in play)"""
    g = golden
    d, step, nonhybrid, l2, L, _ = CASES["repeats"]
    V = {k: v.astype(np.float64) for k, v in case_init(g, "repeats").items()}
    seq, target = g["repeats_seq"][0][:8], g["repeats_target"][0][:8]
    ce, reg, G = P.loss_and_grads(V, seq, target, step, l2, nonhybrid)
    rs = np.random.RandomState(1)
    h = 1e-6
    for name in P.NAMES:
        flat = V[name].reshape(-1)
        picks = rs.choice(flat.size, 3, replace=False).tolist()
        if name == "embedding":
            picks += [int(seq[0][0]) * d, int(target[0]) * d + 1]           # a node's row and a target's row
        for i in picks:
            old = flat[i]
            flat[i] = old + h
            up = sum(P.loss_and_grads(V, seq, target, step, l2, nonhybrid)[:2])
            flat[i] = old - h
            down = sum(P.loss_and_grads(V, seq, target, step, l2, nonhybrid)[:2])
            flat[i] = old
            fd, got = (up - down) / (2 * h), G[name].reshape(-1)[i]
            assert abs(fd - got) <= 1e-6 * max(abs(got), 1e-3), (name, i, fd, got)


def test_sessions_are_independent_and_pad_ids_end_them():
    tab = P.init_tables(9, 4, seed=2)
    seq = np.asarray([[1, 2, 1, 9, 9], [3, 9, 5, 5, 5], [9, 9, 9, 9, 9]])
    both = P.forward(tab, seq, 2)
    alone = P.forward(tab, seq[1:2], 2)
    assert np.array_equal(both[1], alone[0])
    assert np.array_equal(both[1], P.forward(tab, np.asarray([[3, 9, 9, 9, 9]]), 2)[0])     # what follows the pad is unread
    assert not both[2].any()                                                                 # the empty session


# ------------------------------------------------------------------ the epoch order and the schedule
def test_train_samples_and_epoch_feeds_equal_the_recorded_epoch(golden):
    from neurec_amd.model.sequential_recommender.SRGNN import epoch_feeds, train_samples
    g = golden
    train = _user_dict(g)
    L = CASES["hybrid"][4]
    users, ends, lengths = train_samples(train, L)
    assert len(users) == sum(len(s) - 1 for s in train.values())
    k = int(np.flatnonzero(users == users[0])[-1])           # i = 1 first: the longest session of the first user
    first = train[int(users[0])]
    assert ends[0] == len(first) - 1 and ends[k] == 1 and lengths[0] == min(L, len(first) - 1) and lengths[k] == 1
    state = np.random.get_state()
    try:
        np.random.seed(int(g["epoch_seed"]))
        order = epoch_feeds(lengths, int(g["batch_epoch"]))
    finally:
        np.random.set_state(state)
    assert np.array_equal(order, g["epoch_order"])
    assert np.array_equal(users[order], g["epoch_users"]) and np.array_equal(ends[order], g["epoch_ends"])
    assert len(order) < -(-len(users) // 16)                  # drop_last cut the chunks' tails


def test_learning_rates_equal_the_trace_across_the_drop(golden):
    from neurec_amd.model.sequential_recommender.SRGNN import learning_rates
    g = golden
    n = sum(len(s) - 1 for s in _user_dict(g).values())
    step = float(g["epoch_lr_dc_step"])
    lrs = learning_rates(0.001, 0.1, step, n, 20, 0, 4)
    assert lrs.dtype == np.float32 and np.array_equal(lrs, g["hybrid_lrs"])
    S = len(g["epoch_lrs"])
    got = learning_rates(0.001, 0.1, step, n, 16, 0, S)
    assert np.array_equal(got, g["epoch_lrs"]) and len(set(got.tolist())) > 3
    assert np.array_equal(learning_rates(0.001, 0.1, step, n, 16, 5, S - 5), got[5:])       # global_step carries over
    assert np.array_equal(P.learning_rates(0.001, 0.1, 2.0, 4), g["hybrid_lrs"])
    # staircase, not continuous: the second step still has the first rate
    assert lrs[1] == lrs[0] and lrs[2] < lrs[1]


# ------------------------------------------------------------------ the maker
def test_the_makers_shim_ops_and_the_reference_s_creation_order():
    """tests/golden/make_golden_srgnn.py attaches the ops SRGNN.py needs beyond the shim's and checks each on a
    hand-computed value; with the reference tree at hand, the class's variables come in creation order.  The shim is
    put back as it was."""
    from oracle import ref_models as rm
    from oracle import tf_shim
    spec = importlib.util.spec_from_file_location("make_golden_srgnn",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_srgnn.py"))
    path = list(sys.path)
    before = dict(vars(tf_shim))
    nn_before, train_before = dict(vars(tf_shim.nn)), dict(vars(tf_shim.train))
    had_shape = hasattr(tf_shim.Tensor, "get_shape")
    try:
        maker = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(maker)
        assert maker.attach_srgnn_ops() is True
        for k in ("gather_nd", "to_int32", "zeros_initializer"):
            assert hasattr(tf_shim, k), k
        assert hasattr(tf_shim.nn, "dynamic_rnn") and hasattr(tf_shim.train, "exponential_decay")
        if rm.available():
            from make_golden_tfgraph import toy_matrix
            R = toy_matrix(isolated=False)
            seqs = maker.time_orders(R)
            ds = maker.TimedDataset(R, seqs)
            maker.build(ds, maker._hyper("gated", 20, maker.count_samples(seqs)), "float64")
            d = CASES["gated"][0]
            got = [tuple(v.value.shape) for v in maker._variables(d)]
            assert got == [P.shapes(I_TOY, d)[n] for n in P.NAMES]
    finally:
        for mod, saved in ((tf_shim, before), (tf_shim.nn, nn_before), (tf_shim.train, train_before)):
            for k in list(vars(mod)):
                if k not in saved:
                    delattr(mod, k)
            for k, v in saved.items():
                setattr(mod, k, v)
        if not had_shape and hasattr(tf_shim.Tensor, "get_shape"):
            del tf_shim.Tensor.get_shape
        tf_shim._GRAPH.__dict__.pop("collections", None)
        tf_shim.set_float("float32")
        tf_shim.reset_default_graph()
        sys.path[:] = path


# ------------------------------------------------------------------ the plugin and the engine on the host
def test_find_recommender_resolves_srgnn():
    from neurec_amd.main import find_recommender
    from neurec_amd.model.AbstractRecommender import SeqAbstractRecommender
    cls = find_recommender("SRGNN")
    assert cls.__module__ == "neurec_amd.model.sequential_recommender.SRGNN" and issubclass(cls, SeqAbstractRecommender)
    assert "Deviations" in sys.modules[cls.__module__].__doc__


def test_the_plugin_reads_the_reference_s_config_keys():
    from neurec_amd.model.sequential_recommender import SRGNN as mod
    import inspect
    src = inspect.getsource(mod.SRGNN.__init__)
    keys = re.findall(r'config\["(\w+)"\]', src)
    assert keys == ["lr", "L2", "hidden_size", "step", "batch_size", "epochs", "lr_dc", "lr_dc_step", "nonhybrid",
                    "max_seq_len"]
    assert list(inspect.signature(mod.SRGNN.__init__).parameters) == ["self", "sess", "dataset", "config"]


def test_the_defaults_row_equals_the_reference_s_properties_file(tmp_path):
    """defaults.MODELS["SRGNN"] against the copy of the reference's conf/SRGNN.properties under tests/golden/"""
    from neurec_amd import defaults
    ref = configparser.ConfigParser()
    ref.optionxform = str
    assert ref.read(os.path.join(GOLDEN, "neurec_conf", "conf", "SRGNN.properties"))
    want = dict(ref["hyperparameters"])
    assert list(want) == ["lr", "L2", "hidden_size", "batch_size", "epochs", "lr_dc", "lr_dc_step", "step", "nonhybrid",
                          "max_seq_len"]
    assert dict(defaults.MODELS["SRGNN"]) == want and [k for k, _ in defaults.MODELS["SRGNN"]] == list(want)
    path = defaults.write_default_configs(str(tmp_path))
    from neurec_amd.util.configurator import Configurator
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=SRGNN"])
    finally:
        os.chdir(cwd)
    assert (conf["lr"], conf["L2"], conf["hidden_size"], conf["batch_size"], conf["epochs"]) == (0.001, 1e-5, 64, 100, 500)
    assert (conf["lr_dc"], conf["lr_dc_step"], conf["step"], conf["nonhybrid"], conf["max_seq_len"]) == \
        (0.1, 3, 1, False, 200)


def test_the_initial_values():
    """shapes, ranges, the two bias constants, nasr_b zero and b_in / b_out NOT zero; the same values on every call"""
    from neurec_amd.model.sequential_recommender.SRGNN import initial_values
    from neurec_amd import srgnn
    I, d = 37, 16
    V = initial_values(I, d)
    assert list(V) == list(P.NAMES) == list(srgnn.TABLES)
    stdv = 1.0 / np.sqrt(d)
    for name, v in V.items():
        assert v.dtype == np.float32 and v.shape == P.shapes(I, d)[name] == srgnn.shapes(I, d)[name], name
    for name in ("nasr_w1", "nasr_w2", "nasrv", "embedding", "W_in", "b_in", "W_out", "b_out", "B"):
        assert np.abs(V[name]).max() <= stdv and np.abs(V[name]).max() > 0.5 * stdv and V[name].std() > 0.3 * stdv, name
    assert not V["nasr_b"].any() and not V["candidate_bias"].any()
    assert (V["gates_bias"] == 1.0).all()                                     # a gate bias of ones, not zeros
    for name, (rows, cols) in (("gates_kernel", (3 * d, 2 * d)), ("candidate_kernel", (3 * d, d))):
        lim = np.sqrt(6.0 / (rows + cols))
        assert 0.9 * lim < np.abs(V[name]).max() <= lim, name
    again = initial_values(I, d)
    assert all(np.array_equal(V[k], again[k]) for k in V)
    assert not np.array_equal(V["W_in"], V["W_out"])


def test_the_plugin_refuses_a_multi_rank_run_by_name(monkeypatch):
    from neurec_amd import parallel
    from neurec_amd.model.sequential_recommender.SRGNN import SRGNN
    model = SRGNN.__new__(SRGNN)
    many = type("Comm", (), {"active": True, "rank": 0, "world": 2})()
    monkeypatch.setattr(parallel, "get_comm", lambda: many)
    with pytest.raises(NotImplementedError, match="SRGNN runs on one GPU"):
        model.build_graph()


def test_the_engine_refuses_shapes_by_name():
    """refused before a device is asked for"""
    from neurec_amd.srgnn import SRGNNEngine
    for d, L, step, batch, I, text in ((129, 5, 1, 4, 9, r"hidden_size=129 is not supported \(1 to 128\)"),
                                       (4, 257, 1, 4, 9, r"max_seq_len=257 is not supported \(1 to 256\)"),
                                       (4, 0, 1, 4, 9, r"max_seq_len=0 is not supported \(1 to 256\)"),
                                       (4, 5, 5, 4, 9, r"step=5 is not supported \(1 to 4\)"),
                                       (4, 5, 0, 4, 9, r"step=0 is not supported \(1 to 4\)"),
                                       (4, 5, 1, 4097, 9, r"batch_size=4097 is not supported \(1 to 4096\)"),
                                       (4, 5, 1, 0, 9, r"batch_size=0 is not supported \(1 to 4096\)"),
                                       (4, 5, 1, 4096, 1 << 19, r"batch_size \* num_items = 2147483648 is not supported")):
        tab = {k: np.zeros(s, np.float32) for k, s in P.shapes(I, d).items()}
        with pytest.raises(NotImplementedError, match=text):
            SRGNNEngine(tab, 0.001, 0.0, batch, L, step)


def test_the_header_declares_the_entries_and_lib_binds_them():
    from neurec_amd import _lib, build, srgnn
    with open(os.path.join(ROOT, "include", "neurec_hip.h")) as f:
        text = f.read()
    for name in ("nrhip_srgnn_step", "nrhip_srgnn_forward", "nrhip_srgnn_workspace_floats"):
        assert re.search(r"^int %s\(" % name, text, re.M) and name in _lib.SIGNATURES, name
        above = re.findall(r"^/\*.*?\*/", text[:text.index("int %s(" % name)], re.S | re.M)[-1]
        assert re.search(r"[Rr]eplaces", above), name
    assert re.search(r"#define NRHIP_ABI_VERSION 4\b", text)
    for macro, value in (("MAX_WIDTH", srgnn.MAX_WIDTH), ("MAX_LEN", srgnn.MAX_LEN), ("MAX_STEP", srgnn.MAX_STEP),
                         ("MAX_BATCH", srgnn.MAX_BATCH)):
        assert re.search(r"#define NRHIP_SRGNN_%s %d\b" % (macro, value), text), macro
    for struct, cls, lead, tail in (
            ("nrhip_srgnn_weights", _lib.SrgnnWeights, [], ["n_items", "d", "L", "step", "nonhybrid"]),
            ("nrhip_srgnn_feed", _lib.SrgnnFeed, [], ["n_users"]),
            ("nrhip_srgnn_step_args", _lib.SrgnnStepArgs, ["w", "f"], ["batch", "l2"])):
        block = text[text.index("typedef struct %s {" % struct):text.index("} %s;" % struct)]
        names = lead + re.findall(r"\*\s*d_(\w+);", block)
        fields = [n for n, _ in cls._fields_]
        assert fields[:len(names)] == names and fields[len(names):] == tail, struct
    assert "srgnn.hip" in build.SOURCES
    assert tuple(_lib.SRGNN_VARS) == P.NAMES


def test_the_c_entries_refuse_by_name():
    """the bounds of the C entries (host code of the library: no GPU needed, nothing is launched)"""
    from neurec_amd import _lib
    floats = C.c_size_t(0)
    for args, text in (((8, 5, 129, 1, 9), r"hidden_size 129 outside 1\.\.128"),
                       ((8, 257, 4, 1, 9), r"max_seq_len 257 outside 1\.\.256"),
                       ((8, 5, 4, 5, 9), r"step 5 outside 1\.\.4"), ((8, 5, 4, 0, 9), r"step 0 outside 1\.\.4"),
                       ((4097, 5, 4, 1, 9), r"batch_size 4097 outside 0\.\.4096"),
                       ((4096, 5, 4, 1, 1 << 19), r"batch_size \* num_items = 2147483648 is not supported")):
        with pytest.raises(NotImplementedError, match=text):
            _lib.call("nrhip_srgnn_workspace_floats", *args, C.byref(floats))
    _lib.call("nrhip_srgnn_workspace_floats", 8, 5, 4, 2, 9, C.byref(floats))
    assert floats.value >= 8 * 5 * 4 * (3 + 2 * 8) + 8 * 9           # H, X, GATE, ... per iteration, and the logits
    a = _lib.SrgnnStepArgs()
    a.w.d, a.w.L, a.w.step, a.w.n_items, a.batch = 4, 5, 1, 9, 4097
    with pytest.raises(NotImplementedError, match=r"batch_size 4097 outside 0\.\.4096"):
        _lib.call("nrhip_srgnn_step", C.byref(a), None)
    a.batch = 2
    with pytest.raises(ValueError, match="null weight pointer"):
        _lib.call("nrhip_srgnn_step", C.byref(a), None)
    w, f = _lib.SrgnnWeights(), _lib.SrgnnFeed()
    w.d, w.L, w.step, w.n_items = 4, 257, 1, 9
    with pytest.raises(NotImplementedError, match="max_seq_len 257 outside"):
        _lib.call("nrhip_srgnn_forward", C.byref(w), C.byref(f), 2, None, None, 4, None)
