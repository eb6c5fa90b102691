"""numpy restatements of the sparse product Y = A·X in the exact order of additions the SpMM kernels document
(neurec_amd/csrc/spmm_blocked.hip, spmm.hip), and the graph cases the CPU and GPU row tests share.

Every product a·x and every sum is rounded on its own (`acc + a * x` on float32 arrays; the kernels use __fmul_rn /
__fadd_rn), and every chain is written with np.add.accumulate, which adds strictly one element after the other.  Each
function takes dtype=np.float64 for the reference of the same order.

Where a sum starts (the kernel lines that settle it):
  * spmm_blocked_kernel: an entry {slot, length, begin, row} starts from the row's accumulator s_acc[slot] when
    slot < r_max and from +0 otherwise ("if (live && slot < kRMax) acc = s_acc[...]; // segments start from zero"); the
    accumulators are zeroed once, before the first phase, so a later phase goes on from the stored value; after the
    phase a combine record {row slot, first partial, segments, row} starts from the ROW's accumulator
    ("float4 acc = s_acc[cm.x * LPR + c]") and adds the partial slots in slot order.
  * spmm_staged_masked_kernel (one phase only): staged_walk's retire() starts every entry from +0 ("if (r.first) acc =
    0") and writes a row-slot entry straight out; its combine starts from +0 ("float4 acc = make_float4(0...)").  In one
    phase the row accumulator of a cut row is +0, so both give the same bits: lane_group() restates both.
  * spmm_wanted_rows_kernel: the same staged_walk over the w_* schedule (slot 0: the whole row, else partial slot
    slot - r_max); the w_cmb record {row, first, segments} starts from +0.  The chunked path (w_nnz_cap) changes when
    a sub-list is staged, not what is added to what.
  * spmm_wanted_wave_kernel: ww_sublist_sum starts a sub-list from +0 (lane group 0: "acc = carry" with carry = zero)
    and hands the running sum from lane group to lane group; slot 0 writes the row, -(1 + s) is LDS partial s, added
    from +0 by the ww_lcmb record of the same workgroup, 1 + s is global partial s; ww_chunk_done lets the workgroup
    that reports a hub's last chunk add ALL the hub's partials from +0 in segment order ("float4 sum = 0; for s0 ...").
    WHICH workgroup that is depends on timing; what it adds does not (every partial is read back from memory, its own
    included), so the result does not depend on the finishing order.
  * spmm.hip (work items): rows of <= 256 non-zeros are one chain from +0; a longer row is cut into 256-long segments
    (kSegLen, a constant: nrhip_spmm_plan_create's item_rows / item_nnz only group WHOLE rows of <= 256 into work
    items and never change a segment's length), each summed from +0, and the row is p0 + p1 + ... starting from p0
    itself (spmm_fix_kernel: "acc[c] = partial[first ...]; for (s = 1; ...)"; hub_row_block: "total = (s0 == 0 &&
    w == 0) ? pv : total + pv").
A chain that starts from +0 can never hold -0 under round-to-nearest (+0 + -0 = +0, x + -x = +0), so "from +0" and
"from the first partial" give the same bits, and a skipped term equals an added zero: the masks change nothing else.

No intermediate value of any case may be subnormal (the kernels' flush-to-zero mode is then no part of a bit
comparison): every chain asserts it."""
import numpy as np
import scipy.sparse as sp

TINY = float(np.finfo(np.float32).tiny)
CANARY = np.float32(-7.25)


def _no_subnormal(a):
    a = np.abs(a)
    assert not ((a > 0) & (a < TINY)).any(), "a subnormal intermediate value"


class _Terms:
    """the rounded products a[j] * X[col[j]] of every stored entry, in storage order, and which of them are skipped"""

    def __init__(self, A, X, dtype, x_row_nonzero=None):
        self.dtype, self.d = dtype, X.shape[1]
        self.prod = A.data.astype(dtype)[:, None] * X.astype(dtype)[A.indices]
        _no_subnormal(self.prod)
        self.keep = None if x_row_nonzero is None else np.asarray(x_row_nonzero)[A.indices] != 0
        self.zero = np.zeros(self.d, dtype)

    def chain(self, start, b, e):
        """((start + p[b]) + p[b + 1]) + ... + p[e - 1], skipped terms left out"""
        p = self.prod[b:e] if self.keep is None else self.prod[b:e][self.keep[b:e]]
        if len(p) == 0:
            return start.copy()
        run = np.add.accumulate(np.concatenate([start[None], p]), axis=0, dtype=self.dtype)
        _no_subnormal(run)
        return run[-1]

    def chain_of(self, start, parts):
        run = np.add.accumulate(np.concatenate([start[None], parts]), axis=0, dtype=self.dtype)
        _no_subnormal(run)
        return run[-1]


def sequential(A, X, dtype=np.float32, x_row_nonzero=None):
    """every row in storage order, from +0"""
    T = _Terms(A, X, dtype, x_row_nonzero)
    Y = np.zeros((A.shape[0], T.d), dtype)
    for r in range(A.shape[0]):
        Y[r] = T.chain(T.zero, A.indptr[r], A.indptr[r + 1])
    return Y


def lane_group(P, A, X, dtype=np.float32, x_row_nonzero=None):
    """the main schedule of a host plan: workgroup by workgroup, phase by phase (spmm_blocked_kernel plain / MASKED /
    ADAM; spmm_staged_masked_kernel on one-phase plans)"""
    T = _Terms(A, X, dtype, x_row_nonzero)
    n, K, n_wg, r_max, p_max = A.shape[0], P["n_phases"], P["n_wg"], P["r_max"], P["p_max"]
    ent, cmb = P["ent"].astype(np.int64), P["cmb"].astype(np.int64)
    eoff, coff = P["ent_off"].reshape(n_wg, K + 1), P["cmb_off"].reshape(n_wg, K + 1)
    pk, row_of = P["pk_dst"].astype(np.int64), P["row_of"]
    pos_of_row = np.empty(n, np.int64)
    pos_of_row[row_of] = np.arange(n)
    Y = np.zeros((n, T.d), dtype)
    seen = np.zeros(n, bool)
    for w in range(n_wg):
        r0, nr = int(P["wg_row0"][w]), int(P["wg_nrows"][w])
        s = np.zeros((r_max + p_max, T.d), dtype)              # zeroed once: a later phase goes on from the stored sum
        for k in range(K):
            written = set()
            for slot, length, begin, row in ent[eoff[w, k]:eoff[w, k + 1]]:
                assert 0 <= slot < r_max + p_max and slot not in written      # lane groups run side by side
                written.add(int(slot))
                b = (begin & 0xFFFFFFFF) - pk[pos_of_row[row]] + A.indptr[row]
                s[slot] = T.chain(s[slot] if slot < r_max else T.zero, b, b + length)
            for rslot, first, ns, row in cmb[coff[w, k]:coff[w, k + 1]]:
                assert rslot < r_max <= first and first + ns <= r_max + p_max and rslot not in written
                s[rslot] = T.chain_of(s[rslot], s[first:first + ns])
        rows = row_of[r0:r0 + nr]
        assert not seen[rows].any()
        seen[rows] = True
        Y[rows] = s[:nr]
    assert seen.all()
    return Y


def wanted_rows(P, A, X, dtype=np.float32):
    """the w_* schedule (spmm_wanted_rows_kernel); needs P["wanted_ok"]"""
    assert P["wanted_ok"]
    T = _Terms(A, X, dtype)
    n, n_wg, r_max, p_max = A.shape[0], P["n_wg"], P["r_max"], P["p_max"]
    ent, cmb = P["w_ent"].astype(np.int64), P["w_cmb"].astype(np.int64)
    eoff, coff = P["w_ent_off"].reshape(n_wg, 2), P["w_cmb_off"].reshape(n_wg, 2)
    Y = np.zeros((n, T.d), dtype)
    seen = np.zeros(n, bool)
    for w in range(n_wg):
        part = np.zeros((p_max, T.d), dtype)
        for slot, length, begin, row in ent[eoff[w, 0]:eoff[w, 1]]:
            b = begin & 0xFFFFFFFF
            acc = T.chain(T.zero, b, b + length)
            if slot == 0:
                assert not seen[row]
                Y[row], seen[row] = acc, True
            else:
                part[slot - r_max] = acc
        for row, first, ns, _ in cmb[coff[w, 0]:coff[w, 1]]:
            assert not seen[row]
            Y[row], seen[row] = T.chain_of(T.zero, part[first - r_max:first - r_max + ns]), True
    assert seen.all()
    return Y


def wanted_wave(P, A, X, dtype=np.float32):
    """the ww_* schedule (spmm_wanted_wave_kernel and its hub combine); needs P["ww_ok"]"""
    assert P["ww_ok"]
    T = _Terms(A, X, dtype)
    n, n_wg = A.shape[0], P["n_wg"]
    ent, off, lcoff = P["ww_ent"].astype(np.int64), P["ww_off"], P["ww_lcoff"]
    Y = np.zeros((n, T.d), dtype)
    seen = np.zeros(n, bool)
    glob = np.zeros((max(P["ww_segments"], 1), T.d), dtype)
    for w in range(n_wg):
        lds = np.zeros((max(P["ww_lds_slots"], 1), T.d), dtype)
        for slot, length, begin, row in ent[off[w]:off[w + 1]]:
            b = begin & 0xFFFFFFFF
            acc = T.chain(T.zero, b, b + length)
            if slot == 0:
                assert not seen[row]
                Y[row], seen[row] = acc, True
            elif slot < 0:
                lds[-slot - 1] = acc
            else:
                glob[slot - 1] = acc
        for row, first, ns, _ in P["ww_lcmb"].astype(np.int64)[lcoff[w]:lcoff[w + 1]]:
            assert not seen[row]
            Y[row], seen[row] = T.chain_of(T.zero, lds[first:first + ns]), True
    for row, first, ns, _ in P["ww_hub"].astype(np.int64):          # by whichever workgroup reports the last chunk
        assert not seen[row]
        Y[row], seen[row] = T.chain_of(T.zero, glob[first:first + ns]), True
    assert seen.all()
    return Y


def work_item(A, X, seg=256, dtype=np.float32, x_row_nonzero=None):
    """spmm.hip: 256-long segments of a longer row from +0 each, then p0 + p1 + ... starting from p0"""
    T = _Terms(A, X, dtype, x_row_nonzero)
    Y = np.zeros((A.shape[0], T.d), dtype)
    for r in range(A.shape[0]):
        b, e = int(A.indptr[r]), int(A.indptr[r + 1])
        if e - b <= seg:
            Y[r] = T.chain(T.zero, b, e)
        else:
            parts = np.stack([T.chain(T.zero, s, min(s + seg, e)) for s in range(b, e, seg)])
            Y[r] = T.chain_of(parts[0], parts[1:])
    return Y


def cut_rows(P, which):
    """the rows a schedule cuts: those a combine record names"""
    if which == "main":
        return np.unique(P["cmb"][:, 3])
    if which == "wanted":
        return np.unique(P["w_cmb"][:, 0])
    return np.unique(np.concatenate([P["ww_lcmb"][:, 0], P["ww_hub"][:, 0]]))


def epilogue(y, addend=None, sum_in=None, layer_a=None, layer_b=None):
    """(Y, sum_out): Y = y + addend; sum_out = ((sum_in + layer_a) + layer_b) + Y, every term optional"""
    dt = y.dtype
    if addend is not None:
        y = y + addend.astype(dt)
    if sum_in is None:
        return y, None
    s = sum_in.astype(dt)
    if layer_a is not None:
        s = s + layer_a.astype(dt)
    if layer_b is not None:
        s = s + layer_b.astype(dt)
    out = s + y
    _no_subnormal(y)
    _no_subnormal(out)
    return y, out


def keep_canary(produced, wanted, rows_beyond=2):
    """what an output buffer pre-filled with CANARY holds after a call that produces the rows with wanted != 0 only
    (None: every row): `produced` there, the canary elsewhere and in the rows beyond n_rows"""
    out = np.full((produced.shape[0] + rows_beyond, produced.shape[1]), CANARY, produced.dtype)
    sel = slice(None) if wanted is None else np.asarray(wanted) != 0
    out[:produced.shape[0]][sel] = produced[sel]
    return out


def zero_rows(X, x_row_nonzero):
    """the operand a column mask promises: rows with flag 0 are zero"""
    X = X.copy()
    X[np.asarray(x_row_nonzero) == 0] = 0
    return X


# ---- the graph cases --------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025]


def _signed_values(rng, n):
    """signed, |v| in [0.5, 2]"""
    return ((0.5 + 1.5 * rng.rand(n)) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)).astype(np.float32)


def _csr(rows, cols, vals, shape):
    """CSR in the given storage order (rows ascending; no sorting, no merging — stored zeros stay)"""
    rows = np.asarray(rows, np.int64)
    assert (np.diff(rows) >= 0).all()
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=shape[0]))]).astype(np.int64)
    return sp.csr_matrix((np.asarray(vals, np.float32), np.asarray(cols, np.int32), indptr), shape=shape)


def case_lengths():
    """N = 1100, one row of each length in LENGTHS (the 16-entry chunk, the 64- and 256-segment boundaries), rows
    spread over the matrix, a few stored zeros; column 3 of X is the all-zero row (x_zero_rows)"""
    rng = np.random.RandomState(101)
    n = 1100
    at = 7 + 61 * np.arange(len(LENGTHS))                                  # 7, 68, ... 1044: apart, not a tile multiple
    rows, cols = [], []
    for r, k in zip(at, LENGTHS):
        c = np.sort(rng.choice(n, k, replace=False))
        if k >= 15:
            c[0] = 3                                                       # the zero row of X is gathered by every row
            c = np.unique(c)
            while len(c) < k:
                c = np.unique(np.append(c, rng.randint(0, n)))
        rows += [r] * k
        cols += c.tolist()
    vals = _signed_values(rng, len(rows))
    vals[[5, 40, 700, 2000, 3900]] = 0.0                                   # stored zeros
    A = _csr(rows, cols, vals, (n, n))
    assert sorted(np.diff(A.indptr)[at].tolist()) == LENGTHS and A.nnz == sum(LENGTHS)
    return dict(A=A, split=0, hubs=at[np.array(LENGTHS) > 64], x_zero_rows=[3], factors=False)


def case_tiny():
    """the 5 x 5, three-entry matrix of test_spmm_empty_rows_and_tiny"""
    A = sp.csr_matrix((np.array([1.5, -2.0, 0.5], np.float32), (np.array([0, 0, 3]), np.array([1, 4, 2]))), shape=(5, 5))
    A.sort_indices()
    return dict(A=A, split=0, hubs=np.zeros(0, np.int64), x_zero_rows=[], factors=False)


def case_star(n=2049):
    """N = 2049: row 0 holds the other 2048 columns (32 segments: four 8-segment chunks of the wave-cooperative hop),
    every other row holds column 0.  N = 3330 ("star_wide"): 53 segments, more than a d = 256 plan has partial slots
    on any number of workgroups — the planner refuses it and the work-item kernel remains"""
    rng = np.random.RandomState(103)
    rows = [0] * (n - 1) + list(range(1, n))
    cols = list(range(1, n)) + [0] * (n - 1)
    return dict(A=_csr(rows, cols, _signed_values(rng, len(rows)), (n, n)), split=0, hubs=np.array([0]),
                x_zero_rows=[], factors=False)


BIP_U, BIP_I = 300, 200


def _bip_pairs():
    rng = np.random.RandomState(107)
    u, i = [], []
    for user in range(BIP_U):
        items = set(rng.choice(np.arange(2, BIP_I), rng.randint(0, 31), replace=False).tolist())
        for hub in (0, 1):                                                 # two hub items taken by 90 % of the users
            if rng.rand() < 0.9:
                items.add(hub)
        items = sorted(items)
        u += [user] * len(items)
        i += items
    return np.array(u), np.array(i)


def case_bipartite(kind):
    """U = 300, I = 200, 0-30 items per user, two hub items: lightgcn_adjacency as pre / norm, the transpose of norm,
    and gcmc in descending storage order"""
    from neurec_amd.graph import lightgcn_adjacency, transpose_csr
    u, i = _bip_pairs()
    if kind == "descending":
        A = lightgcn_adjacency(u, i, BIP_U, BIP_I, "gcmc", tf_order=True)
    elif kind == "norm_t":
        A = transpose_csr(lightgcn_adjacency(u, i, BIP_U, BIP_I, "norm"))
    else:
        A = lightgcn_adjacency(u, i, BIP_U, BIP_I, kind)
    A = sp.csr_matrix((A.data.astype(np.float32), A.indices.astype(np.int32), A.indptr.astype(np.int64)), shape=A.shape)
    lens = np.diff(A.indptr)
    assert (lens[BIP_U:BIP_U + 2] > 256).all()
    return dict(A=A, split=BIP_U, hubs=np.flatnonzero(lens > 64), x_zero_rows=[], factors=kind in ("pre", "descending"))


def case_cap():
    """the five-heavy-rows case of test_spmm_plan_cpu.test_accumulator_cap_binds (r_max = 20, p_max = 8 on 8
    workgroups), with signed values"""
    rng = np.random.RandomState(11)
    rows, cols = [], []
    for u, k in enumerate([60] * 5 + [1] * 150):
        it = np.sort(rng.choice(400, k, replace=False))
        rows += [u] * k
        cols += (155 + it).tolist()
    A = _csr(rows, cols, _signed_values(rng, len(rows)), (155, 555))
    return dict(A=A, split=0, hubs=np.zeros(0, np.int64), x_zero_rows=[], factors=False)


def case_heavy():
    """64 rows x 200 non-zeros, N = 256: every row is a hub of four 64-segments"""
    rng = np.random.RandomState(109)
    n = 256
    rows, cols = [], []
    for r in range(64):
        rows += [4 * r] * 200
        cols += np.sort(rng.choice(n, 200, replace=False)).tolist()
    return dict(A=_csr(rows, cols, _signed_values(rng, len(rows)), (n, n)), split=0, hubs=4 * np.arange(64),
                x_zero_rows=[], factors=False)


def case_short():
    """12,000 rows x 2 non-zeros (d = 16 on 8 workgroups: row lists longer than a workgroup has threads)"""
    rng = np.random.RandomState(113)
    n = 12000
    cols = np.stack([rng.randint(0, n // 2, n), rng.randint(n // 2, n, n)], 1).ravel()
    return dict(A=_csr(np.repeat(np.arange(n), 2), cols, _signed_values(rng, 2 * n), (n, n)), split=0,
                hubs=np.zeros(0, np.int64), x_zero_rows=[], factors=False)


CASES = {"lengths": case_lengths, "tiny": case_tiny, "star": case_star, "cap": case_cap, "heavy": case_heavy,
         "short": case_short, "star_wide": lambda: case_star(3330), "pre": lambda: case_bipartite("pre"), "norm": lambda: case_bipartite("norm"),
         "norm_t": lambda: case_bipartite("norm_t"), "descending": lambda: case_bipartite("descending")}
_MADE = {}


def case(name):
    """the case, built once per process; never modified"""
    if name not in _MADE:
        c = CASES[name]()
        c["name"] = name
        assert c["A"].nnz <= 60000
        _MADE[name] = c
    return _MADE[name]


def operand(c, d, seed=0):
    """X = randn [n_cols][d] with the case's zero rows"""
    X = np.random.RandomState(1000 + seed + d).randn(c["A"].shape[1], d).astype(np.float32)
    X[c["x_zero_rows"]] = 0
    return X


# ---- the (case, width, workgroups, options) combinations the row tests run -----------------------------------------------
# options: the planner's own arguments (waves, seg, r_max, p_max, split), the switches a plan's creation reads from the
# environment (masked_fast, wanted_wave, wanted_nnz_cap), "phases": k (a block_bytes that cuts the columns into k
# blocks), "min_rp": the smallest r_max, then the smallest p_max, the planner accepts for the case, "gif4": the
# gathers-in-flight = 4 instantiation, "refuse": the planner's message where it refuses the combination.
def _c(name, d, n_wg, **kw):
    return (name, d, n_wg, kw)


def _d64(name, n_wg, n_wg8, split=0):
    s = dict(split=split) if split else {}
    return [_c(name, 64, n_wg, **s), _c(name, 64, n_wg8, waves=8, **s), _c(name, 64, n_wg, seg=16, **s),
            _c(name, 64, n_wg, seg=32, **s), _c(name, 64, n_wg, phases=2, **s), _c(name, 64, n_wg, phases=4, **s),
            _c(name, 64, n_wg, min_rp=True, **s), _c(name, 64, n_wg, seg=16, min_rp=True, wanted_wave=0, **s),
            _c(name, 64, n_wg, gif4=True, **s), _c(name, 64, n_wg, masked_fast=0, **s),
            _c(name, 64, n_wg, wanted_wave=0, **s), _c(name, 64, n_wg, masked_fast=0, wanted_wave=0, **s),
            _c(name, 64, n_wg, wanted_wave=0, wanted_nnz_cap=300, **s)]


COMBOS = _d64("lengths", 8, 8) + _d64("star", 8, 16) + _d64("pre", 8, 8, split=BIP_U) + [
    _c("pre", 64, 8), _c("norm", 64, 8, split=BIP_U), _c("norm", 64, 8), _c("norm_t", 64, 8, split=BIP_U),
    _c("descending", 64, 8, split=BIP_U), _c("descending", 64, 8, phases=2), _c("tiny", 64, 8),
    _c("tiny", 64, 8, waves=8), _c("cap", 64, 8, r_max=20, p_max=8), _c("cap", 64, 8, r_max=20, p_max=8, wanted_wave=0),
    _c("heavy", 64, 8, p_max=32), _c("heavy", 64, 8, p_max=32, wanted_wave=0),
    _c("heavy", 64, 8, p_max=31, refuse="more than 31 hub segments in one workgroup phase"),
    _c("star", 64, 8, waves=8, refuse="2049 rows do not fit 8 workgroups x 208 accumulators"),
    # the other widths: the full pass and the general masked kernel
    _c("lengths", 16, 8), _c("lengths", 16, 8, waves=8), _c("lengths", 16, 8, phases=2), _c("lengths", 16, 8, seg=16),
    _c("lengths", 16, 8, gif4=True), _c("lengths", 32, 8), _c("lengths", 32, 8, seg=32, waves=8),
    _c("lengths", 32, 8, phases=4), _c("lengths", 128, 16), _c("lengths", 128, 16, waves=8, phases=2),
    _c("lengths", 256, 16), _c("lengths", 256, 16, min_rp=True),
    _c("lengths", 256, 8, refuse="1100 rows do not fit 8 workgroups x 104 accumulators"),
    _c("star", 16, 8), _c("star", 32, 8, seg=32), _c("star", 128, 16, phases=2), _c("star", 256, 24),
    _c("star", 256, 8, refuse="2049 rows do not fit 8 workgroups x 104 accumulators"),
    _c("pre", 16, 8, split=BIP_U), _c("pre", 32, 8, split=BIP_U, phases=4), _c("pre", 128, 8, split=BIP_U),
    _c("pre", 256, 8, split=BIP_U), _c("norm_t", 16, 8, waves=8), _c("descending", 32, 8, split=BIP_U),
    _c("pre", 256, 8, split=BIP_U, waves=8, refuse="300 rows do not fit 3 workgroups x 52 accumulators"),
    _c("pre", 256, 8, split=BIP_U, seg=16, refuse="more than 48 hub segments in one workgroup phase"),
    _c("heavy", 256, 8, waves=8, refuse="more than 24 hub segments in one workgroup phase"),
    _c("short", 16, 8), _c("short", 16, 8, gif4=True),
    _c("short", 16, 8, waves=8, refuse="12000 rows do not fit 8 workgroups x 832 accumulators"),
]


def combo_id(combo):
    name, d, n_wg, kw = combo
    return "-".join([name, "d%d" % d, "wg%d" % n_wg] + ["%s%s" % (k, "" if v is True else v) for k, v in sorted(kw.items())
                                                      if k != "refuse"] + (["refused"] if "refuse" in kw else []))


PLANNER_KEYS = ("waves", "seg", "r_max", "p_max", "masked_fast", "wanted_wave", "wanted_nnz_cap")


def planner_args(build, lib, combo):
    """the explicit arguments of spmm_plan_host.build for a combination (phases and min_rp resolved on the host)"""
    name, d, n_wg, kw = combo
    A = case(name)["A"]
    args = dict(split_row=kw.get("split", 0))
    args.update({k: kw[k] for k in PLANNER_KEYS if k in kw})
    if "phases" in kw:
        span = int(A.indices.max()) + 1 - int(A.indices.min())
        args["block_bytes"] = (span * d * 4 + kw["phases"] - 1) // kw["phases"]
    if kw.get("min_rp"):
        args["r_max"], args["p_max"] = smallest_accumulators(build, lib, A, d, n_wg, args)
    return args


def smallest_accumulators(build, lib, A, d, n_wg, args):
    """the smallest r_max the planner accepts with its default partial slots, then the smallest p_max with that r_max"""
    def accepted(**more):
        try:
            build(lib, A, d, n_wg, **dict(args, **more))
            return True
        except Exception as e:
            if not hasattr(e, "code"):
                raise
            return False
    r = next(r for r in range(max(A.shape[0] // n_wg, 1), A.shape[0] + 2) if accepted(r_max=r))
    p = next(p for p in range(1, 4096) if accepted(r_max=r, p_max=p))
    return r, p


def dispatch(P, form):
    """the kernel nrhip_spmm_blocked's dispatch reaches for a plan and a masked form ("rows", "cols", "both"), or the
    full pass ("full")"""
    wide = "spmm_blocked_kernel<%s, %d waves>" % ("masked" if form != "full" else "plain", P["waves"])
    if form == "full":
        return wide
    if form == "rows":
        if P["ww_ok"]:
            return "spmm_wanted_wave_kernel"
        if P["wanted_ok"]:
            return "spmm_wanted_rows_kernel"
    if P["colmask_ok"]:
        return "spmm_staged_masked_kernel<%s>" % {"rows": "rows", "cols": "cols", "both": "cols, rows"}[form]
    return wide


def phases_word(P):
    return "one phase" if P["n_phases"] == 1 else "several phases"
