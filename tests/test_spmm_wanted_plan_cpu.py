"""The per-batch work lists of the planned batch-rows hop (neurec_amd/csrc/spmm_wanted_plan.h) checked on the CPU.
tests/hostcheck/wantedplancheck.cpp is the g++ build of the header the device planner shares its sort key, slot counts
and item encoders with; plan_batch is the host statement of what spmm_wanted_epoch_plan_kernel writes
(tests/test_spmm_wanted_planned_gpu.py compares the two byte for byte).

What spmm_wanted_planned_kernel relies on:
  * every non-zero of every batch row is in exactly one item, no other row appears, an empty row still gets its item;
  * the segments of a 65..512 row are consecutive, in order, inside one workgroup (16 items) and carry their count;
  * a hub's segments are consecutive and in order, its chunks of 8 start on a multiple of 8, each chunk head names the
    hub, and the chunk heads of a hub are as many as the planner's record says;
  * the item count stays within the stride, which depends on the graph and the batch size only;
  * the list is a pure function of its inputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG, CHUNK, WAVES = 64, 8, 16


@pytest.fixture(scope="module")
def wp():
    d = os.path.join(ROOT, "tests", "hostcheck")
    so, src = os.path.join(d, "libwantedplancheck.so"), os.path.join(d, "wantedplancheck.cpp")
    csrc = os.path.join(ROOT, "neurec_amd", "csrc")
    hdrs = [os.path.join(csrc, "spmm_wanted_plan.h"), os.path.join(csrc, "spmm_blocked_plan.h")]
    if (not os.path.isfile(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", csrc, "-o", so, src])
    lib = C.CDLL(so)
    lib.wp_stride.argtypes = [C.c_void_p, C.c_int64, C.c_int]
    lib.wp_stride.restype = C.c_int64
    lib.wp_items_bound.argtypes = [C.c_void_p, C.c_int64, C.c_int]
    lib.wp_items_bound.restype = C.c_int64
    lib.wp_plan_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_int64)]
    lib.wp_plan_batch.restype = C.c_int64
    return lib


def graph(rng, n_rows, special):
    """row lengths: mostly short with a heavy tail, `special` lengths planted at the front"""
    lens = np.minimum((rng.pareto(1.1, n_rows) * 6).astype(np.int64), 3000)
    lens[:len(special)] = special
    indptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    return indptr


def batch_keys(rng, indptr, n_users, B, force_rows=()):
    """sorted occurrence keys of a batch as nrhip_bpr_plan leaves them: users, then items offset by n_users; positives
    drawn by degree (hubs always among them), repeated rows included"""
    n_rows = len(indptr) - 1
    deg = np.diff(indptr)[n_users:].astype(np.float64) + 0.01
    users = rng.randint(0, n_users, B)
    pos = n_users + rng.choice(n_rows - n_users, B, p=deg / deg.sum())
    neg = n_users + rng.randint(0, n_rows - n_users, B)
    forced = np.asarray(force_rows, np.int64)[:B]
    users[:len(forced)] = np.where(forced < n_users, forced, users[:len(forced)])
    pos[:len(forced)] = np.where(forced >= n_users, forced, pos[:len(forced)])
    rows = np.concatenate([users, pos, neg]).astype(np.uint64)
    keys = (rows << np.uint64(32)) | np.arange(3 * B, dtype=np.uint64)
    return np.sort(keys)


def plan(lib, indptr, keys, B):
    n_rows = len(indptr) - 1
    stride = lib.wp_stride(indptr.ctypes.data, n_rows, B)
    out = np.full((stride, 4), 7, np.int32)
    hubs = np.zeros((n_rows, 4), np.int32)
    nh = C.c_int64(0)
    n = lib.wp_plan_batch(indptr.ctypes.data, n_rows, keys.ctypes.data, len(keys), stride, out.ctypes.data,
                          hubs.ctypes.data, C.byref(nh))
    return n, stride, out, hubs[:nh.value]


def check(indptr, keys, n, stride, out, hubs, B):
    rows = np.unique((keys >> np.uint64(32)).astype(np.int64))
    lens = np.diff(indptr)
    assert 0 <= n <= stride - 1 and (stride - 1) % WAVES == 0
    assert tuple(out[0]) == (n, len(rows), 0, 0)
    items = out[1:1 + n]
    assert (out[1 + n:, 3] == -1).all() and (out[1 + n:, :3] == 0).all()
    covered = {}                                     # row -> list of (first, length) in item order
    hub_of_row = {int(h[0]): (i, h) for i, h in enumerate(hubs)}
    heads = {}
    i = 0
    while i < n:
        x, y, z, w = (int(v) for v in items[i])
        if w == -1:
            assert (x, y, z) == (0, 0, 0)
            i += 1
            continue
        ln = int(lens[w])
        assert w not in covered, "row %d appears in two places" % w
        if x == 0:
            assert ln <= SEG and y == ln and z == indptr[w]
            covered[w] = [(z, y)]
            i += 1
        elif x < 0:
            ns = (ln + SEG - 1) // SEG
            assert 2 <= ns <= CHUNK
            assert i // WAVES == (i + ns - 1) // WAVES, "a row's segments cross a workgroup"
            segs = []
            for sg in range(ns):
                xs, ys, zs, ws = (int(v) for v in items[i + sg])
                assert ws == w and -xs - 1 == sg + 16 * ns and 0 < ys <= SEG
                segs.append((zs, ys))
            covered[w] = segs
            i += ns
        else:
            hub, h = hub_of_row[w]
            ns = int(h[2])
            assert ns == (ln + SEG - 1) // SEG > CHUNK and int(h[3]) == (ns + CHUNK - 1) // CHUNK
            assert i % CHUNK == 0, "a hub's first chunk does not start on a multiple of 8"
            segs, nheads = [], 0
            for sg in range(ns):
                xs, ys, zs, ws = (int(v) for v in items[i + sg])
                assert ws == w and xs == 1 + int(h[1]) + sg and 0 < (ys & 255) <= SEG
                if sg % CHUNK == 0:
                    assert (ys >> 8) == hub + 1
                    nheads += 1
                else:
                    assert (ys >> 8) == 0
                segs.append((zs, ys & 255))
            assert nheads == int(h[3]), "chunk count differs from the planner's record"
            heads[w] = nheads
            covered[w] = segs
            i += ns
    assert sorted(covered) == sorted(int(r) for r in rows), "wanted rows and scheduled rows differ"
    for w, segs in covered.items():
        pos = int(indptr[w])
        for z, y in segs:                            # consecutive CSR positions: every non-zero once, in order
            assert z == pos
            pos += y
        assert pos == indptr[w + 1]
    # descending cost: slot class, then non-zeros (capped), then row id
    order = []
    for k in range(n):
        w = int(items[k][3])
        if w >= 0 and (not order or order[-1] != w):
            order.append(w)

    def slots(ln):
        ns = max(1, (ln + SEG - 1) // SEG)
        return (ns + CHUNK - 1) // CHUNK * CHUNK if ns > CHUNK else (1 if ns <= 1 else 2 if ns <= 2 else 4 if ns <= 4 else 8)
    keyf = [(-min(slots(int(lens[w])), 8), -min(int(lens[w]), 1023), w) for w in order]
    assert keyf == sorted(keyf)


SPECIAL = [0, 1, 64, 65, 128, 129, 512, 513, 1024, 4097, 5000, 0, 63, 511]


@pytest.mark.parametrize("B", [1, 7, 256, 1024, 4096])
def test_every_wanted_nonzero_once_and_chunks_adjacent(wp, B):
    rng = np.random.RandomState(B)
    n_users = 3000
    indptr = graph(rng, 9000, SPECIAL)
    # the planted lengths sit in user rows 0..13; plant the same among the items
    lens = np.diff(indptr)
    lens[n_users:n_users + len(SPECIAL)] = SPECIAL
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    forced = list(range(len(SPECIAL))) + list(range(n_users, n_users + len(SPECIAL)))
    keys = batch_keys(rng, indptr, n_users, B, forced)
    n, stride, out, hubs = plan(wp, indptr, keys, B)
    assert n >= 0
    check(indptr, keys, n, stride, out, hubs, B)
    n2, _, out2, _ = plan(wp, indptr, keys, B)
    assert n2 == n and out2.tobytes() == out.tobytes()


def test_short_last_batch_and_repeated_rows(wp):
    rng = np.random.RandomState(5)
    indptr = graph(rng, 4000, SPECIAL)
    B = 512
    stride = wp.wp_stride(indptr.ctypes.data, 4000, B)
    for nb in (B, 37, 1):                            # the last batch of a stream is short: same stride
        keys = batch_keys(rng, indptr, 1500, nb, list(range(len(SPECIAL))))
        if nb > 4:                                   # the same triplet several times
            rows = (keys >> np.uint64(32))
            rows[:] = np.sort(np.concatenate([rows[:nb // 2], rows[:nb // 2], rows[:len(rows) - 2 * (nb // 2)]]))
            keys = (rows << np.uint64(32)) | np.arange(len(rows), dtype=np.uint64)
        out = np.zeros((stride, 4), np.int32)
        n = wp.wp_plan_batch(indptr.ctypes.data, 4000, keys.ctypes.data, len(keys), stride, out.ctypes.data, None, None)
        assert 0 <= n <= stride - 1
        _, _, out_full, hubs = plan(wp, indptr, keys, B)
        assert out_full.tobytes() == out.tobytes()
        check(indptr, keys, n, stride, out, hubs, B)


def test_stride_is_the_cost_of_the_most_expensive_rows(wp):
    rng = np.random.RandomState(9)
    indptr = graph(rng, 5000, SPECIAL)
    lens = np.diff(indptr)

    def slots(ln):
        ns = max(1, (ln + SEG - 1) // SEG)
        return (ns + CHUNK - 1) // CHUNK * CHUNK if ns > CHUNK else (1 if ns <= 1 else 2 if ns <= 2 else 4 if ns <= 4 else 8)
    sl = np.sort(np.array([slots(int(x)) for x in lens]))[::-1]
    for B in (1, 100, 1024, 4096):
        want = int(sl[:min(3 * B, len(sl))].sum())
        assert wp.wp_items_bound(indptr.ctypes.data, 5000, B) == want
        assert wp.wp_stride(indptr.ctypes.data, 5000, B) == 1 + (want + WAVES - 1) // WAVES * WAVES
    # the batch that wants exactly the most expensive rows meets the bound
    top = np.argsort(-np.array([slots(int(x)) for x in lens]), kind="stable")[:300].astype(np.uint64)
    keys = np.sort((top << np.uint64(32)) | np.arange(300, dtype=np.uint64))
    n, stride, out, hubs = plan(wp, indptr, keys, 100)
    assert n == wp.wp_items_bound(indptr.ctypes.data, 5000, 100)
    check(indptr, keys, n, stride, out, hubs, 100)
