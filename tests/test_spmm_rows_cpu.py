"""tests/spmm_restatement.py pinned on the CPU, on every (graph case, width, planner options) combination
tests/test_spmm_rows_gpu.py runs on the device: the float32 walks of a host plan (tests/spmm_plan_host.py) equal the
sequential row sums in bits on every row the plan does not cut, differ from them on hub rows (so the order of a hub's
additions is observable), stay within the 4 x rule of their float64 forms, and the sequential sums are
oracle.train.spmm_rowwise's.  No intermediate value is subnormal: the restatement asserts it in every chain.  The last
test reads off the host plans which kernel each combination reaches on the device, so that the combination table
provably covers every branch of the dispatch."""
import collections
import functools

import numpy as np
import pytest

import spmm_restatement as R
from spmm_plan_host import Refused, build, load_plancheck

ACCEPTED = [c for c in R.COMBOS if "refuse" not in c[3]]
REFUSED = [c for c in R.COMBOS if "refuse" in c[3]]


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _within(what, got32, want64, seq32, seq64):
    """|got32 - want64| <= 4 x (sequential float32's own distance to float64) + 1e-5 max|want|
    (tests/test_primitives_gpu.py::_within's rule)"""
    err, bar = np.abs(got32.astype(np.float64) - want64).max(), np.abs(seq32.astype(np.float64) - seq64).max()
    assert err <= 4 * bar + 1e-5 * np.abs(want64).max(), (what, err, bar)


@functools.lru_cache(maxsize=None)
def _sequential(name, d):
    c = R.case(name)
    X = R.operand(c, d)
    return R.sequential(c["A"], X), R.sequential(c["A"], X, np.float64)


def _plan(combo):
    name, d, n_wg, _ = combo
    lib = load_plancheck()
    return build(lib, R.case(name)["A"], d, n_wg, **R.planner_args(build, lib, combo))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_sequential_is_the_oracle_and_work_item_cuts_at_256(name):
    from oracle.train import spmm_rowwise
    c = R.case(name)
    A, lens = c["A"], np.diff(c["A"].indptr)
    for d in (16, 64):
        X = R.operand(c, d)
        seq32, seq64 = _sequential(name, d)
        assert _bits_equal(seq32, spmm_rowwise(A, X))
        wi = R.work_item(A, X)
        assert _bits_equal(wi[lens <= 256], seq32[lens <= 256])
        _within(name, wi, R.work_item(A, X, dtype=np.float64), seq32, seq64)
        if name == "lengths":
            differs = (wi.view(np.int32) != seq32.view(np.int32)).any(1)
            assert differs[lens > 256].any() and not differs[lens <= 256].any()
        # a column mask: the skipped terms are zeros, so the masked walk of the zeroed operand has the plain walk's bits
        keep = (np.random.RandomState(5).rand(A.shape[1]) < 0.5).astype(np.uint8)
        Xz = R.zero_rows(X, keep)
        assert _bits_equal(R.sequential(A, Xz, x_row_nonzero=keep), R.sequential(A, Xz))
        assert _bits_equal(R.work_item(A, Xz, x_row_nonzero=keep), R.work_item(A, Xz))


@pytest.mark.parametrize("combo", ACCEPTED, ids=R.combo_id)
def test_the_walks_equal_sequential_off_the_cut_rows(combo):
    name, d, n_wg, kw = combo
    c = R.case(name)
    A, X = c["A"], R.operand(c, d)
    P = _plan(combo)
    if "phases" in kw:
        assert P["n_phases"] == kw["phases"] or (kw.get("split") and P["n_phases"] > 1)
    seq32, seq64 = _sequential(name, d)
    walks = [("main", R.lane_group)]
    if P["wanted_ok"]:
        walks.append(("wanted", R.wanted_rows))
    if P["ww_ok"]:
        walks.append(("wave", R.wanted_wave))
    hub_differs = False
    for which, walk in walks:
        got = walk(P, A, X)
        uncut = np.ones(A.shape[0], bool)
        uncut[R.cut_rows(P, which)] = False
        assert _bits_equal(got[uncut], seq32[uncut]), which
        _within((R.combo_id(combo), which), got, walk(P, A, X, np.float64), seq32, seq64)
        hub_differs |= bool((got.view(np.int32) != seq32.view(np.int32)).any())
    if name == "lengths":
        assert hub_differs                               # the order of a hub's additions shows in the bits
    if kw.get("min_rp"):                                 # one accumulator / one partial slot less is refused
        lib = load_plancheck()
        args = R.planner_args(build, lib, combo)
        for less, msg in ((dict(r_max=args["r_max"] - 1), "accumulators"), (dict(p_max=args["p_max"] - 1), "hub segments")):
            if min(less.values()) >= 1:
                with pytest.raises(Refused) as e:
                    build(lib, A, d, n_wg, **dict(args, **less))
                assert msg in str(e.value)


def test_the_masked_walk_of_a_plan_skips_zeros_only():
    c = R.case("lengths")
    A, X = c["A"], R.operand(c, 64)
    keep = (np.random.RandomState(6).rand(A.shape[1]) < 0.4).astype(np.uint8)
    Xz = R.zero_rows(X, keep)
    for combo in (R.COMBOS[0], [k for k in ACCEPTED if k[0] == "lengths" and k[3].get("phases") == 4][0]):
        P = _plan(combo)
        assert _bits_equal(R.lane_group(P, A, Xz, x_row_nonzero=keep), R.lane_group(P, A, Xz))


def test_column_blocks_cut_a_hub_differently_from_the_wave_schedule():
    """with several phases the full pass cuts a hub per column block, the wave-cooperative schedule by position: the
    two orders differ in bits on hub rows and nowhere else (include/neurec_hip.h says so at nrhip_spmm_csr_masked)"""
    c = R.case("lengths")
    A, X = c["A"], R.operand(c, 64)
    P = _plan([k for k in ACCEPTED if k[0] == "lengths" and k[1] == 64 and k[3].get("phases") == 2][0])
    assert P["ww_ok"] and P["n_phases"] == 2
    differs = (R.lane_group(P, A, X).view(np.int32) != R.wanted_wave(P, A, X).view(np.int32)).any(1)
    assert differs.any() and not differs[np.diff(A.indptr) <= 64].any()


@pytest.mark.parametrize("combo", REFUSED, ids=R.combo_id)
def test_the_refusals_are_the_planner_s(combo):
    with pytest.raises(Refused) as e:
        _plan(combo)
    assert e.value.code == 2 and combo[3]["refuse"] in str(e.value) and "use the work-item kernel" in str(e.value)


def test_the_combinations_reach_every_branch_of_the_dispatch(capsys):
    """nrhip_spmm_blocked's dispatch read off the host plans (R.dispatch restates it): ww_ok, wanted_ok, colmask_ok and
    neither, 8 and 16 waves, one and several phases — every kernel is reached by at least one combination"""
    reached = collections.Counter()
    for combo in ACCEPTED:
        P = _plan(combo)
        for form in ("full", "rows", "cols", "both"):
            reached[R.dispatch(P, form) + ", " + R.phases_word(P)] += 1
        if combo[3].get("gif4"):
            reached["gathers in flight = 4"] += 1
    with capsys.disabled():
        for k in sorted(reached):
            print("%4d  %s" % (reached[k], k))
    need = ["spmm_wanted_wave_kernel, one phase", "spmm_wanted_wave_kernel, several phases",
            "spmm_wanted_rows_kernel, one phase", "spmm_staged_masked_kernel<rows>, one phase",
            "spmm_staged_masked_kernel<cols>, one phase", "spmm_staged_masked_kernel<cols, rows>, one phase",
            "gathers in flight = 4"]
    need += ["spmm_blocked_kernel<%s, %d waves>, %s" % (m, w, k)
             for m in ("plain", "masked") for w in (8, 16) for k in ("one phase", "several phases")]
    assert all(reached[k] > 0 for k in need), [k for k in need if not reached[k]]
