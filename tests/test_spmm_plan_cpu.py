"""The lane-group SpMM schedule (neurec_amd/csrc/spmm_blocked_plan.h) checked on the CPU: the planner is integer work on
indptr / indices, so everything the kernels of spmm_blocked.hip rely on can be asserted from its arrays alone, without a
device.  tests/hostcheck/plancheck.cpp is the g++ build of the very header nrhip_spmm_blocked_plan_create calls; the
workgroup count is passed explicitly (the C entry would ask the device for its CU count).

What a kernel relies on, per schedule:
  * spmm_blocked_kernel / spmm_staged_masked_kernel: row_of lists every row once, a workgroup's rows are
    row_of[wg_row0 : wg_row0 + wg_nrows] (<= r_max accumulators), the packed pairs follow that order, and the entries
    (sub-lists <= seg, hub segments in partial slots r_max .. r_max + p_max, added by the combine records) visit every
    non-zero exactly once, each in the phase of its column block;
  * spmm_wanted_rows_kernel (w_*) and spmm_wanted_wave_kernel (ww_*): the same coverage over CSR positions, their own
    slot encodings, and caps that bound the LDS arrays they index."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from spmm_plan_host import MAX_LDS, ROOT, UNSUPPORTED, Refused, build, load_plancheck


@pytest.fixture(scope="module")
def plancheck():
    return load_plancheck()


# ---- the invariants -------------------------------------------------------------------------------------------------

def check_rows(P, A):
    """row_of is a permutation; wg_row0 / wg_nrows tile it; <= r_max rows each; with a split, one side per workgroup"""
    n = A.shape[0]
    assert P["n_rows"] == n and P["nnz"] == A.nnz
    assert np.array_equal(np.sort(P["row_of"]), np.arange(n))
    nr, r0 = P["wg_nrows"].astype(np.int64), P["wg_row0"].astype(np.int64)
    assert len(nr) == P["n_wg"] and (nr >= 0).all() and nr.max() <= P["r_max"]
    assert np.array_equal(r0, np.concatenate([[0], np.cumsum(nr)[:-1]])) and nr.sum() == n
    wg_of_pos = np.repeat(np.arange(P["n_wg"]), nr)
    if P["split_row"]:
        side = (P["row_of"] >= P["split_row"]).astype(np.int64)
        lo = np.full(P["n_wg"], 2), np.full(P["n_wg"], -1)
        np.minimum.at(lo[0], wg_of_pos, side)
        np.maximum.at(lo[1], wg_of_pos, side)
        assert (lo[0][nr > 0] == lo[1][nr > 0]).all()
    # packed order: running sum of the row lengths in row_of order; pk_src is the row's CSR start
    lens = np.diff(A.indptr)[P["row_of"]]
    assert np.array_equal(P["pk_dst"].astype(np.int64), np.concatenate([[0], np.cumsum(lens)]))
    assert np.array_equal(P["pk_src"].astype(np.int64), A.indptr[P["row_of"]])
    # the workgroup's slice of the packed pairs
    assert np.array_equal(P["wg_nnz"][0::2].astype(np.int64), P["pk_dst"][r0].astype(np.int64))
    assert np.array_equal(P["wg_nnz"][1::2].astype(np.int64), P["pk_dst"][r0 + nr].astype(np.int64) - P["pk_dst"][r0])
    assert P["nnz_cap"] == P["wg_nnz"][1::2].max()
    return wg_of_pos


def tiles_exactly(begin, length, row, row_begin, row_end, total):
    """the pieces (begin, length) with length > 0 cover [0, total) once, each inside its row's range"""
    keep = length > 0
    b, l, r = begin[keep], length[keep], row[keep]
    o = np.argsort(b, kind="stable")
    b, l, r = b[o], l[o], r[o]
    if total == 0:
        assert len(b) == 0
        return
    assert b[0] == 0 and np.array_equal(b[1:], (b + l)[:-1]) and b[-1] + l[-1] == total
    assert (b >= row_begin[r]).all() and (b + l <= row_end[r]).all()


def check_main(P, A):
    wg_of_pos = check_rows(P, A)
    n, K, n_wg, seg, r_max, p_max = A.shape[0], P["n_phases"], P["n_wg"], P["seg"], P["r_max"], P["p_max"]
    ent, cmb = P["ent"].astype(np.int64), P["cmb"].astype(np.int64)
    eoff, coff = P["ent_off"].reshape(n_wg, K + 1).astype(np.int64), P["cmb_off"].reshape(n_wg, K + 1).astype(np.int64)
    for off, tot in ((eoff, len(ent)), (coff, len(cmb))):
        flat = off.ravel()                                             # offsets run on from workgroup to workgroup
        assert flat[0] == 0 and flat[-1] == tot and (np.diff(off, axis=1) >= 0).all()
        assert np.array_equal(off[1:, 0], off[:-1, K])
    assert (eoff[:, K] - eoff[:, 0]).max() <= P["ent_cap"] and P["ent_cap"] % 16 == 0
    e_wg = np.repeat(np.arange(n_wg), eoff[:, K] - eoff[:, 0])
    e_ph = np.repeat(np.tile(np.arange(K), n_wg), np.diff(eoff, axis=1).ravel())
    slot, length, begin, row = ent[:, 0], ent[:, 1], ent[:, 2] & 0xFFFFFFFF, ent[:, 3]
    assert (length >= 0).all() and (length <= seg).all() and (row >= 0).all() and (row < n).all()
    # the owner is a row of the entry's workgroup; a non-hub entry's slot is the row's place in that workgroup's list
    pos_of_row = np.empty(n, np.int64)
    pos_of_row[P["row_of"]] = np.arange(n)
    assert np.array_equal(wg_of_pos[pos_of_row[row]], e_wg)
    hub = slot >= r_max
    assert np.array_equal(slot[~hub], (pos_of_row[row] - P["wg_row0"][e_wg])[~hub])
    assert (slot[hub] < r_max + p_max).all()
    # coverage: every packed position once, inside the owner's packed range
    pk = P["pk_dst"].astype(np.int64)
    tiles_exactly(begin, length, row, pk[pos_of_row], pk[pos_of_row + 1], A.nnz)
    # rows without non-zeros still get an (empty) entry: their accumulator is written out
    seen = np.zeros(n, bool)
    seen[row] = True
    assert seen.all()
    # column blocks: all columns of a phase-k entry lie inside block k of its class
    live = length > 0
    csr0 = begin - pk[pos_of_row[row]] + A.indptr[row]
    first_col, last_col = A.indices[csr0[live]], A.indices[(csr0 + length - 1)[live]]
    for ra, rb in ([(0, P["split_row"]), (P["split_row"], n)] if P["split_row"] else [(0, n)]):
        cols = A.indices[A.indptr[ra]:A.indptr[rb]]
        cmin, cmax = (int(cols.min()), int(cols.max())) if len(cols) else (0, 0)
        span = cmax + 1 - cmin
        kk = max((span * P["d"] * 4 + (P["block_bytes"] or 1 << 40) - 1) // (P["block_bytes"] or 1 << 40), 1)
        width = (span + kk - 1) // kk
        m = (row[live] >= ra) & (row[live] < rb)
        assert np.array_equal((first_col[m] - cmin) // width, e_ph[live][m])
        assert np.array_equal((last_col[m] - cmin) // width, e_ph[live][m])
        assert (e_ph[~live & (row >= ra) & (row < rb)] == 0).all()
    # within a (workgroup, phase): non-increasing length, partial slots unique
    same = (e_wg[1:] == e_wg[:-1]) & (e_ph[1:] == e_ph[:-1])
    assert (length[1:][same] <= length[:-1][same]).all()
    key = (e_wg[hub] * K + e_ph[hub]) * (r_max + p_max) + slot[hub]
    assert len(np.unique(key)) == len(key)
    # combine records: {row slot, first partial slot, segments, row}: the row's hub sub-list of that phase, cut into
    # `segments` consecutive pieces (all `seg` long but the last) that sit in consecutive partial slots
    c_wg = np.repeat(np.arange(n_wg), coff[:, K] - coff[:, 0])
    c_ph = np.repeat(np.tile(np.arange(K), n_wg), np.diff(coff, axis=1).ravel())
    assert cmb[:, 2].sum() == hub.sum()
    where = {int(k): i for k, i in zip(key, np.flatnonzero(hub))}
    for (rslot, first, ns, crow), w, k in zip(cmb, c_wg, c_ph):
        assert ns >= 2 and r_max <= first and first + ns <= r_max + p_max
        assert rslot == pos_of_row[crow] - P["wg_row0"][w]
        idx = [where[int((w * K + k) * (r_max + p_max) + first + s)] for s in range(ns)]     # KeyError: slot missing
        assert (row[idx] == crow).all() and (length[idx][:-1] == seg).all()
        assert np.array_equal(begin[idx][1:], (begin[idx] + length[idx])[:-1])


def check_wanted(P, A):
    """staged wanted-rows schedule: spmm_wanted_rows_kernel stages a sub-list with one wave (length <= 64, packed into
    8 bits), keeps at most w_ent_cap descriptors in each of two LDS lists, puts partial sums at slot - r_max"""
    n, n_wg, seg, r_max, p_max = A.shape[0], P["n_wg"], P["seg"], P["r_max"], P["p_max"]
    if not P["wanted_ok"]:
        return False
    ent, cmb = P["w_ent"].astype(np.int64), P["w_cmb"].astype(np.int64)
    eoff, coff = P["w_ent_off"].reshape(n_wg, 2).astype(np.int64), P["w_cmb_off"].reshape(n_wg, 2).astype(np.int64)
    for off, tot in ((eoff, len(ent)), (coff, len(cmb))):
        assert off[0, 0] == 0 and off[-1, 1] == tot and np.array_equal(off[1:, 0], off[:-1, 1]) and (off[:, 1] >= off[:, 0]).all()
    assert (eoff[:, 1] - eoff[:, 0]).max() <= P["w_ent_cap"]
    slot, length, begin, row = ent[:, 0], ent[:, 1], ent[:, 2] & 0xFFFFFFFF, ent[:, 3]
    assert (length >= 0).all() and (length <= min(seg, 64, 255)).all() and (row >= 0).all() and (row < n).all()
    assert P["w_nnz_cap"] >= 4 * seg                                   # any sub-list fits the staging buffer alone
    assert P["p_max"] * 256 + 2 * P["w_ent_cap"] * 16 + P["w_bitmap_words"] * 4 + P["w_nnz_cap"] * 8 <= MAX_LDS
    assert P["w_bitmap_words"] == 0 or P["w_bitmap_words"] * 32 >= n
    tiles_exactly(begin, length, row, A.indptr[:-1].astype(np.int64), A.indptr[1:].astype(np.int64), A.nnz)
    whole = slot == 0
    assert np.array_equal(length[whole], np.diff(A.indptr)[row[whole]])         # slot 0: the whole row, written directly
    assert len(np.unique(row[whole])) == whole.sum()
    assert ((slot[~whole] >= r_max) & (slot[~whole] < r_max + p_max)).all()
    e_wg = np.repeat(np.arange(n_wg), eoff[:, 1] - eoff[:, 0])
    key = e_wg[~whole] * (r_max + p_max) + slot[~whole]
    assert len(np.unique(key)) == len(key)
    where = {int(k): i for k, i in zip(key, np.flatnonzero(~whole))}
    c_wg = np.repeat(np.arange(n_wg), coff[:, 1] - coff[:, 0])
    assert cmb[:, 2].sum() == (~whole).sum() and len(np.unique(cmb[:, 0])) == len(cmb)
    for (crow, first, ns, _), w in zip(cmb, c_wg):
        assert ns >= 2 and r_max <= first and first + ns <= r_max + p_max
        idx = [where[int(w * (r_max + p_max) + first + s)] for s in range(ns)]
        assert (row[idx] == crow).all() and begin[idx][0] == A.indptr[crow]
        assert np.array_equal(begin[idx][1:], (begin[idx] + length[idx])[:-1])
        assert begin[idx][-1] + length[idx][-1] == A.indptr[crow + 1]
    seen = np.zeros(n, bool)
    seen[row] = True
    assert seen.all()
    return True


def check_wanted_wave(P, A):
    """wave-cooperative schedule: spmm_wanted_wave_kernel gives a sub-list to one wave (length <= 64); slot 0 writes the
    row, -(1 + s) is LDS partial s (< ww_lds_slots, summed by the ww_lcmb record in the same workgroup), 1 + s is
    global partial s (< ww_segments, summed by whichever of the hub's `chunks` workgroups finishes last)"""
    n, n_wg, seg = A.shape[0], P["n_wg"], P["seg"]
    if not P["ww_ok"]:
        return False
    ent, hubs, lcmb, gch = P["ww_ent"].astype(np.int64), P["ww_hub"].astype(np.int64), P["ww_lcmb"].astype(np.int64), P["ww_gch"]
    off, choff, lcoff = (P[k].astype(np.int64) for k in ("ww_off", "ww_choff", "ww_lcoff"))
    for o, tot in ((off, len(ent)), (choff, len(gch)), (lcoff, len(lcmb))):
        assert len(o) == n_wg + 1 and o[0] == 0 and o[-1] == tot and (np.diff(o) >= 0).all()
    assert np.diff(off).max() <= P["ww_ent_cap"]
    words = (n + 127) // 128 * 4
    assert P["ww_lds_slots"] * 256 + P["ww_ent_cap"] * 16 + words * 4 + 16 <= MAX_LDS and words * 32 >= n
    slot, length, begin, row = ent[:, 0], ent[:, 1], ent[:, 2] & 0xFFFFFFFF, ent[:, 3]
    assert (length >= 0).all() and (length <= min(seg, 64)).all() and (row >= 0).all() and (row < n).all()
    tiles_exactly(begin, length, row, A.indptr[:-1].astype(np.int64), A.indptr[1:].astype(np.int64), A.nnz)
    seen = np.zeros(n, bool)
    seen[row] = True
    assert seen.all()
    e_wg = np.repeat(np.arange(n_wg), np.diff(off))
    whole, lds, glob = slot == 0, slot < 0, slot > 0
    assert np.array_equal(length[whole], np.diff(A.indptr)[row[whole]]) and len(np.unique(row[whole])) == whole.sum()
    # LDS partials: unique per workgroup, below ww_lds_slots, each summed by one record of the same workgroup
    ls = -slot[lds] - 1
    assert (ls < P["ww_lds_slots"]).all() if lds.any() else True
    key = e_wg[lds] * (P["ww_lds_slots"] + 1) + ls
    assert len(np.unique(key)) == len(key)
    where = {int(k): i for k, i in zip(key, np.flatnonzero(lds))}
    l_wg = np.repeat(np.arange(n_wg), np.diff(lcoff))
    assert lcmb[:, 2].sum() == lds.sum() and len(np.unique(lcmb[:, 0])) == len(lcmb)
    for (crow, first, ns, _), w in zip(lcmb, l_wg):
        idx = [where[int(w * (P["ww_lds_slots"] + 1) + first + s)] for s in range(ns)]
        assert (row[idx] == crow).all() and begin[idx][0] == A.indptr[crow]
        assert np.array_equal(begin[idx][1:], (begin[idx] + length[idx])[:-1])
        assert begin[idx][-1] + length[idx][-1] == A.indptr[crow + 1]
    # global partials: slot s of hub {row, first, segments, chunks} is segment s - first of the row; the workgroups
    # that hold its segments name the hub once per chunk of <= 8 consecutive segments, `chunks` times in all
    gs = slot[glob] - 1
    assert len(np.unique(gs)) == len(gs) == P["ww_segments"] and (gs < P["ww_segments"]).all()
    assert hubs[:, 2].sum() == P["ww_segments"] and len(np.unique(hubs[:, 0])) == len(hubs)
    g_of = {int(s): i for s, i in zip(gs, np.flatnonzero(glob))}
    named = {}
    g_wg = np.repeat(np.arange(n_wg), np.diff(choff))
    for hub, w in zip(gch, g_wg):
        named[(int(hub), int(w))] = named.get((int(hub), int(w)), 0) + 1
    for hi, (hrow, first, ns, nch) in enumerate(hubs):
        idx = [g_of[int(first + s)] for s in range(ns)]
        assert (row[idx] == hrow).all() and begin[idx][0] == A.indptr[hrow] and nch == (ns + 7) // 8 and nch >= 2
        assert np.array_equal(begin[idx][1:], (begin[idx] + length[idx])[:-1])
        assert begin[idx][-1] + length[idx][-1] == A.indptr[hrow + 1]
        chunks = {}
        for s, i in enumerate(idx):
            chunks.setdefault(int(e_wg[i]), set()).add(s // 8)
        assert sum(len(c) for c in chunks.values()) == nch                # a chunk's segments stay in one workgroup
        assert {w: len(c) for w, c in chunks.items()} == {w: k for (h, w), k in named.items() if h == hi}
    assert sum(named.values()) == hubs[:, 3].sum()
    return True


def check_layout(P, lib, A):
    """sections in the order the buffer has held them since the arrays were added, each 256-byte aligned, with the tail
    padding the kernels' prefetches may read (a descriptor / an index past the end)"""
    nb = lambda k: P[k].size * P[k].itemsize
    want = [nb("ent") + 16, nb("cmb") + 16, nb("wg_row0"), nb("wg_nrows"), nb("row_of"), nb("pk_src"), nb("pk_dst"),
            A.nnz * 4 + 4, A.nnz * 4 + 4, nb("ent_off"), nb("cmb_off"), nb("wg_nnz"), nb("w_ent") + 16, nb("w_cmb") + 16,
            nb("w_ent_off"), nb("w_cmb_off")]
    if P["ww_ok"]:
        want += [nb("ww_off"), nb("ww_choff"), nb("ww_ent") + 16, nb("ww_gch") + 4, nb("ww_hub") + 16, nb("ww_lcoff"),
                 nb("ww_lcmb") + 16, P["ww_segments"] * 256 + 256, len(P["ww_hub"]) * 4 + 4]
    assert P["sec_size"].tolist() == want
    assert (P["sec_off"] % 256 == 0).all() and P["sec_off"][0] == 0
    assert np.array_equal(P["sec_off"][1:], (P["sec_off"] + (P["sec_size"] + 255) // 256 * 256)[:-1])
    assert P["sec_off"][-1] + P["sec_size"][-1] <= P["used"] <= lib.pc_plan_bytes(A.shape[0], A.nnz)


def check_all(P, lib, A):
    check_main(P, A)
    w, ww = check_wanted(P, A), check_wanted_wave(P, A)
    check_layout(P, lib, A)
    return w, ww


# ---- the matrices ---------------------------------------------------------------------------------------------------

def bipartite(n_users, n_items, degrees, seed):
    """symmetric bipartite adjacency (the shape LightGCN multiplies by): users first, `degrees` per user (capped)"""
    rng = np.random.RandomState(seed)
    rows, cols = [], []
    for u, k in enumerate(degrees):
        it = rng.choice(n_items, min(int(k), n_items), replace=False)
        rows += [u] * len(it)
        cols += (n_users + it).tolist()
    r, c = np.array(rows + cols), np.array(cols + rows)
    A = sp.csr_matrix((np.ones(len(r), np.float32), (r, c)), shape=(n_users + n_items,) * 2)
    A.sum_duplicates()
    A.sort_indices()
    return A


def small_graph(seed, hub=150):
    rng = np.random.RandomState(seed)
    deg = rng.zipf(1.6, 260).clip(0, 40)
    deg[:3] = hub                                   # hub users (sub-lists longer than seg); some users stay empty
    deg[5:9] = 0
    return bipartite(260, 340, deg, seed), 260


@pytest.fixture(scope="module")
def twin():
    """the gowalla-shaped twin of tests/test_spmm_dealt_gpu.py::_graph('degree'): the bench's workload"""
    from neurec_amd import synth
    from neurec_amd.graph import lightgcn_adjacency
    train, _ = synth.interactions_around_test(
        synth.load_test_split(os.path.join(ROOT, "tests", "golden", "gowalla_test_split.npz")), 810128, seed=2018)
    U, I = train.shape
    deg = np.asarray(train.sum(0)).ravel()
    new_of = np.empty(I, np.int64)
    new_of[np.argsort(-deg, kind="stable")] = np.arange(I)
    coo = train.tocoo()
    A = lightgcn_adjacency(coo.row, new_of[coo.col], U, I, "pre").tocsr()
    A.sort_indices()
    return A, U


# ---- the cases ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("waves", [8, 16])
@pytest.mark.parametrize("d", [16, 32, 64, 128, 256])
def test_small_graphs(plancheck, d, waves, split):
    for seed in (1, 2):
        A, U = small_graph(seed, hub=150 if d < 256 else 100)
        P = build(plancheck, A, d, n_wg=24, split_row=U if split else 0, waves=waves)
        assert P["n_phases"] == 1 and P["split_row"] == (U if split else 0)
        w, ww = check_all(P, plancheck, A)
        assert w == ww == (d == 64 and waves == 16)              # the dedicated row-masked kernels are d = 64, 16 waves


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("d", [16, 64, 256])
def test_several_phases(plancheck, d, split):
    A, U = small_graph(3, hub=100)
    P = build(plancheck, A, d, n_wg=24, split_row=U if split else 0, block_bytes=A.shape[0] * d * 4 // 5 + 1)
    assert 3 <= P["n_phases"] <= 5
    assert check_all(P, plancheck, A) == (False, d == 64)        # the staged kernels need one phase; the wave kernel does not


def test_multi_chunk_hubs_and_switches(plancheck):
    """rows of > 8 segments are spread over several workgroups by the wave-cooperative schedule"""
    deg = np.full(300, 3)
    deg[:2] = (1500, 700)
    deg[2] = 512                                                 # exactly 8 segments: one chunk, LDS partials
    A = bipartite(300, 1600, deg, 7)
    P = build(plancheck, A, 64, n_wg=16, split_row=300)
    assert check_all(P, plancheck, A) == (True, True)
    assert len(P["ww_hub"]) == 2 and P["ww_segments"] == 24 + 11 and len(P["ww_lcmb"]) >= 1 and P["colmask_ok"] == 1
    off = build(plancheck, A, 64, n_wg=16, split_row=300, masked_fast=0)
    assert (off["colmask_ok"], off["wanted_ok"], off["ww_ok"]) == (0, 0, 1) and len(off["w_ent"]) == 0
    check_all(off, plancheck, A)
    off = build(plancheck, A, 64, n_wg=16, split_row=300, wanted_wave=0)
    assert (off["colmask_ok"], off["wanted_ok"], off["ww_ok"]) == (1, 1, 0) and len(off["ww_ent"]) == 0
    check_all(off, plancheck, A)
    capped = build(plancheck, A, 64, n_wg=16, split_row=300, wanted_nnz_cap=300)
    assert capped["w_nnz_cap"] == 300 and check_wanted(capped, A)
    assert build(plancheck, A, 64, n_wg=16, split_row=300, wanted_nnz_cap=1)["w_nnz_cap"] == 4 * 64


def test_accumulator_cap_binds(plancheck):
    """five heavy rows and many one-entry rows: equal cost would put 27 rows on three of the workgroups, which have 20
    accumulators — dealing stops at the cap and the rest goes to the other workgroups"""
    A = bipartite(155, 400, [60] * 5 + [1] * 150, 11)[:155].tocsr()      # the user rows alone (rectangular)
    P = build(plancheck, A, 64, n_wg=8, r_max=20, p_max=8)
    assert P["wg_nrows"].max() == 20 and P["wg_nrows"].min() < 20
    check_all(P, plancheck, A)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("d,n_wg", [(64, 256), (16, 256), (256, 1024)])
def test_gowalla_twin(plancheck, twin, d, n_wg, split):
    A, U = twin
    P = build(plancheck, A, d, n_wg=n_wg, split_row=U if split else 0)
    assert check_all(P, plancheck, A) == (d == 64, d == 64)
    if d == 64:
        assert P["colmask_ok"] == 1 and P["w_bitmap_words"] > 0


def test_gowalla_twin_phases(plancheck, twin):
    A, U = twin
    P = build(plancheck, A, 64, n_wg=256, split_row=U, block_bytes=4 << 20)
    assert P["n_phases"] >= 2
    check_all(P, plancheck, A)


def test_refusals(plancheck):
    A, U = small_graph(4)
    with pytest.raises(Refused) as e:                            # 600 rows, 8 workgroups x 52 accumulators
        build(plancheck, A, 256, n_wg=8, waves=8)
    assert e.value.code == UNSUPPORTED and "do not fit 8 workgroups x 52 accumulators" in str(e.value)
    with pytest.raises(Refused) as e:                            # with a split every class must fit its share
        build(plancheck, A, 64, n_wg=8, split_row=U, r_max=60)
    assert e.value.code == UNSUPPORTED and "use the work-item kernel" in str(e.value)
    hubs = bipartite(10, 3000, [64 * 30] + [2] * 9, 5)           # 30 segments in one phase, 24 partial slots
    with pytest.raises(Refused) as e:
        build(plancheck, hubs, 256, n_wg=64, waves=8)
    assert e.value.code == UNSUPPORTED and "more than 24 hub segments in one workgroup phase" in str(e.value)
    with pytest.raises(Refused) as e:                            # 600 rows x 256 B in blocks of 1 KB: 150 blocks
        build(plancheck, A, 64, n_wg=24, block_bytes=1024)
    assert e.value.code == UNSUPPORTED and "column blocks (max 32)" in str(e.value)
    for kw in (dict(d=48), dict(d=64, waves=4), dict(d=64, r_max=1000), dict(d=64, n_wg=4)):
        with pytest.raises(Refused) as e:
            build(plancheck, A, kw.pop("d"), n_wg=kw.pop("n_wg", 24), **kw)
        assert e.value.code == UNSUPPORTED


def test_deterministic(plancheck, twin):
    for A, U, n_wg in ((twin[0], twin[1], 256), small_graph(1) + (24,)):
        a, b = (build(plancheck, A, 64, n_wg=n_wg, split_row=U) for _ in range(2))
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), k
