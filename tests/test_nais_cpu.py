"""NAIS without a GPU: the float64 restatement the GPU tests lean on (tests/nais_restatement.py) against the reference
class's own f64 trace — every step, table and loss, and predict() for both algorithms — and the edges the golden
batches were chosen for, the padding term among them."""
import numpy as np
import pytest

from conftest import load_golden
import fism_restatement as F
import nais_restatement as NA

# case -> (loss, learner, pairwise); algorithm / activation / alpha / beta are in the fixture (<case>_hyper)
CASES = {"a0_none_ce": ("cross_entropy", "adam", False), "a0_relu_square": ("square", "adam", False),
         "a1_tanh": ("square", "adam", False), "a0_sigmoid_b1": ("square", "adam", False),
         "gd": ("square", "gd", False), "adagrad": ("square", "adagrad", False),
         "rmsprop": ("square", "rmsprop", False), "momentum": ("square", "momentum", False),
         "bpr": ("bpr", "adam", True)}


@pytest.fixture(scope="module")
def golden():
    return NA.load_trace(load_golden)


def make_state(g, case, dtype=np.float64):
    _, learner, _ = CASES[case]
    alg = int(g[case + "_hyper"][0])
    return NA.State(g["c1_0"], g["Q0"], g["bias_0"], g["W0_a%d" % alg], g["b_0"], g["h_0"], learner=learner,
                    lr=float(g["learning_rate"]), dtype=dtype)


def test_cases_are_the_fixture_s(golden):
    assert sorted(CASES) == sorted(str(c) for c in golden["cases"])
    hy = {c: NA.golden_hyper(golden, c) for c in CASES}
    assert hy["a0_none_ce"] == dict(algorithm=0, activation=-1, alpha=0.0, beta=0.5)       # the shipped config
    assert hy["a0_relu_square"]["activation"] == 0 and hy["a0_relu_square"]["alpha"] == 0.5
    assert hy["a1_tanh"]["algorithm"] == 1 and hy["a1_tanh"]["activation"] == 2
    assert hy["a0_sigmoid_b1"]["activation"] == 1 and hy["a0_sigmoid_b1"]["beta"] == 1.0
    assert not np.all(golden["h_0"] == 1.0) and np.abs(golden["b_0"]).min() > 0.25


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_the_f64_trace(golden, case):
    """every step of every case: tables and loss within 1e-12 of the reference class's float64 run"""
    g = golden
    loss, _, pairwise = CASES[case]
    hy = NA.golden_hyper(g, case)
    R = F.golden_matrix(g)
    st = make_state(g, case)
    for k in range(len(g[case + "_users"])):
        got = NA.step(st, R, g[case + "_users"][k], g[case + "_items"][k], g[case + "_third"][k], pairwise, loss,
                      g["regs"], **hy)
        assert abs(got - g[case + "_f64_loss"][k]) <= 1e-12 * max(1.0, abs(got)), (k, got)
        for name, want in zip(NA.NAMES, NA.golden_tables(g, case, "f64", k)):
            err = np.abs(st.var[name] - want).max()
            assert err <= 1e-12, (case, k, name, err)
    if case in ("a0_none_ce", "a1_tanh"):
        got = NA.predict(R, [st.var[n] for n in NA.NAMES], g["predict_users"], **hy)
        assert np.abs(got - g["predict_a%d_f64" % hy["algorithm"]]).max() <= 1e-12


def test_the_history_mask_is_another_model(golden):
    """attention_mask="history" drops the padding term: the first step's loss leaves the trace (the term is in the
    reference), and a batch whose histories all have one length is the same under both forms"""
    g = golden
    case = "a0_relu_square"
    loss, _, pairwise = CASES[case]
    hy = NA.golden_hyper(g, case)
    R = F.golden_matrix(g)
    st = make_state(g, case)
    got = NA.step(st, R, g[case + "_users"][0], g[case + "_items"][0], g[case + "_third"][0], pairwise, loss,
                  g["regs"], mask="history", **hy)
    assert abs(got - g[case + "_f64_loss"][0]) > 1e-6
    deg = np.diff(R.indptr)
    users = np.flatnonzero(deg == 3)[:4].astype(np.int32)
    assert len(users) >= 2
    items = np.full(len(users), R.shape[1] - 1, np.int32)
    labels = np.zeros(len(users), np.float32)
    a, b = make_state(g, case), make_state(g, case)
    la = NA.step(a, R, users, items, labels, False, loss, g["regs"], mask="history", **hy)
    lb = NA.step(b, R, users, items, labels, False, loss, g["regs"], mask="reference", **hy)
    assert la == lb and all(np.array_equal(a.var[n], b.var[n]) for n in NA.NAMES)


def test_batches_hold_the_edges(golden):
    """what the golden batches were chosen for: a user twice, an item twice, excluded first / last of the row, an empty
    history (pointwise), histories of 1, 63, 64, 65 and (case a0_none_ce) 1,100 items — and in EVERY step, per side,
    some instances carry the padding term and exactly the longest ones do not"""
    g = golden
    R = F.golden_matrix(g)
    for case, (_, _, pairwise) in CASES.items():
        lens_all = set()
        for k in range(len(g[case + "_users"])):
            inst = F.instances(R, g[case + "_users"][k], g[case + "_items"][k], g[case + "_third"][k], pairwise)
            assert len(inst) <= 64
            users, items = [x[0] for x in inst], [x[1] for x in inst]
            assert len(set(users)) < len(users) and len(set(items)) < len(items)
            lens = {len(F.history(R, u, e)) for u, _, e, _, _ in inst}
            assert {1, 63, 64, 65} <= lens and (pairwise or 0 in lens)
            first = [1 for u, _, e, _, _ in inst if e >= 0 and R.indices[R.indptr[u]] == e]
            last = [1 for u, _, e, _, _ in inst if e >= 0 and R.indices[R.indptr[u + 1] - 1] == e]
            assert first and last
            lens_all |= lens
            sides = [inst] if not pairwise else [inst[:len(inst) // 2], inst[len(inst) // 2:]]
            for s in sides:
                ids, m, _, n, hist = NA.padded(R, s, "reference")
                hl = np.asarray([len(x) for x in hist])
                assert np.array_equal(n, hl + 1)                       # num_idx = |H| + 1
                carries = m.sum(axis=1) > hl                           # a masked position beyond the history
                assert carries.any() and np.array_equal(~carries, hl == hl.max())
                assert np.all(ids[np.arange(len(s))[carries], hl[carries]] == R.shape[1])      # ... holding the pad id
        if case == "a0_none_ce":
            assert max(lens_all) >= 1099
