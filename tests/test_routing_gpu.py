"""The row-sharded routing (neurec_amd/csrc/route.hip, sharded.RowRouter) at any world size, on ONE device in ONE
process: the kernels take `world` as a plain integer, so one GPU computes what each of W ranks would, and the exchange
between the ranks is a permutation numpy does (tests/routing_restatement.py states all of it; tests/test_routing_cpu.py
checks that statement).  No collective is involved: a bug is a failed assertion, never a hang.

Every comparison is exact — integer equality, or bit equality of fp32 sums taken in the order of the concatenated
batch.  Buffers are pre-filled with a sentinel so that what a call must leave alone is seen to be left alone."""
import numpy as np
import pytest

import routing_restatement as R
from routing_restatement import CASES, EPOCH_CASES

pytestmark = pytest.mark.gpu

SENT = -12345            # pre-fill of every output buffer


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def _i32(a):
    return _dev(a, np.int32)


def _host(t):
    return t.cpu().numpy().astype(np.int64)


def _pairs(rows, codes):
    return np.stack([np.asarray(rows, np.int64), np.asarray(codes, np.int64)], 1)


def _out(shape, dtype, fill=SENT):
    import torch
    return torch.full(shape, fill, dtype=dtype, device="cuda")


# ---------------------------------------------------------------------------------------------- the kernels, per rank
@pytest.mark.parametrize("name", sorted(CASES))
def test_route_batch_per_rank_equals_the_restatement(name):
    """nrhip_route_batch for every rank, twice in a row on RowRouter-sized buffers shared by all ranks: junk in the
    counts the first time, the first call's counts the second time; then every empty rank once more right after a
    rank that left non-zero counts behind."""
    import torch
    from neurec_amd import engine as E
    U, I, W, batches = R.make_case(name)
    lay, res = R.Layout(U, I, W), R.restate(U, I, W, batches)
    lens = [len(b[0]) for b in batches]
    cap = max(3 * max(lens), 1)
    keys, packed = _out((cap,), torch.int64), _out((cap, 2), torch.int32)
    order, inv, counts = _out((cap,), torch.int32), _out((cap,), torch.int32), _out((W,), torch.int32)

    def run(r, junk):
        users, pos, neg = (_i32(x) for x in batches[r])
        n = 3 * lens[r]
        for t in (keys, packed, order, inv):
            t.fill_(SENT)
        if junk:
            counts.fill_(77 + r)
        E.route_batch(users, pos, neg, U, lay.bu, lay.bi, R.CODE, W, keys[:n], packed[:n], order[:n], inv[:n], counts)
        for got, f in ((keys, "keys"), (packed, "packed"), (order, "order"), (inv, "inv")):
            h = _host(got)
            np.testing.assert_array_equal(h[:n], res[r][f], err_msg="%s of rank %d" % (f, r))
            assert (h[n:] == SENT).all(), "%s of rank %d: written past 3·B" % (f, r)
        np.testing.assert_array_equal(_host(counts), res[r]["send_counts"], err_msg="counts of rank %d" % r)

    for r in range(W):
        run(r, True)
        run(r, False)
    full = [r for r in range(W) if lens[r] > 0]
    for r in range(W):
        if lens[r] == 0:
            run(full[0], False)
            assert int(counts.sum()) == 3 * lens[full[0]] > 0
            run(r, False)                                            # all zero again, nothing else touched


def test_an_empty_batch_zeroes_the_counts_of_the_batch_before():
    """the entry itself, with batch = 0 and buffers that exist: d_counts must not keep the step before (the plugins hand
    a rank an empty slice whenever the short last batch has fewer triplets than ranks)"""
    import torch
    from neurec_amd import engine as E
    W = 4
    ids, keys, packed = _i32([0]), _out((3,), torch.int64), _out((3, 2), torch.int32)
    order, inv, counts = _out((3,), torch.int32), _out((3,), torch.int32), _out((W,), torch.int32)

    def call(batch):
        E.call("nrhip_route_batch", E._ptr(ids), E._ptr(ids), E._ptr(ids), batch, 10, 3, 2, R.CODE, E._ptr(keys),
               E._ptr(packed), E._ptr(order), E._ptr(inv), E._ptr(counts), W, E._stream())
    call(1)
    assert _host(counts).tolist() == [3, 0, 0, 0]                     # user 0, item 0, item 0: all rank 0's
    for t in (keys, packed, order, inv):
        t.fill_(SENT)
    call(0)
    assert _host(counts).tolist() == [0, 0, 0, 0]
    assert all((_host(t) == SENT).all() for t in (keys, packed, order, inv))


def test_route_batch_takes_empty_tensors():
    """a rank without triplets passes tensors without storage (data_ptr() == 0): a clean return, counts zeroed"""
    import torch
    from neurec_amd import engine as E
    e32 = lambda *s: torch.empty(*s, dtype=torch.int32, device="cuda")
    counts = _out((3,), torch.int32, 9)
    E.route_batch(e32(0), e32(0), e32(0), 10, 4, 3, R.CODE, 3, torch.empty(0, dtype=torch.int64, device="cuda"),
                  e32((0, 2)), e32(0), e32(0), counts)
    assert _host(counts).tolist() == [0, 0, 0]
    E.route_batch(e32(0), e32(0), e32(0), 10, 4, 3, R.CODE, 3, torch.empty(0, dtype=torch.int64, device="cuda"),
                  e32((0, 2)), e32(0), e32(0), None)                   # planned counts: nothing to zero either


def test_route_owner_keys_and_the_sums_take_an_owner_that_is_asked_for_nothing():
    """keys of length 0 have no storage either: clean returns, index_of_pos and the table untouched"""
    import torch
    from neurec_amd import engine as E
    W, G, d = 3, 4, 20
    keys = torch.empty(0, dtype=torch.int64, device="cuda")
    iop = _out((3 * G,), torch.int32)
    E.route_owner_keys(_i32([]), _i32([]), _i32([0] * (W + 1)), _i32([0, 2, 2]), W, G, R.CODE, keys, iop)
    assert (_host(iop) == SENT).all()
    table = _out((5, d), torch.float32, 1.5)
    mine = torch.empty((0, d), dtype=torch.float32, device="cuda")
    E.rows_sum_sorted(keys, iop, mine, table)
    E.rows_sum_sorted2(keys, iop, mine, table, mine, table)
    assert (table.cpu().numpy() == 1.5).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_route_owner_keys_per_owner_equals_the_restatement(name):
    """inputs = the exchange done in numpy; owners that are asked for nothing and sources that send nothing included"""
    import torch
    from neurec_amd import engine as E
    U, I, W, batches = R.make_case(name)
    res = R.restate(U, I, W, batches)
    for t, w in enumerate(res):
        m, G = len(w["asked"]), w["G"]
        keys, iop = _out((m,), torch.int64), _out((3 * G + 2,), torch.int32)
        E.route_owner_keys(_i32(w["asked"]), _i32(w["asked_code"]), _i32(w["recv_prefix"]), _i32(w["size_off"]), W, G,
                           R.CODE, keys, iop)
        np.testing.assert_array_equal(_host(keys), w["okeys"], err_msg="keys of owner %d" % t)
        want = np.where(w["index_of_pos"] == R.FILL, SENT, w["index_of_pos"])
        np.testing.assert_array_equal(_host(iop), np.concatenate([want, [SENT, SENT]]),
                                      err_msg="index_of_pos of owner %d" % t)


@pytest.mark.parametrize("name", sorted(EPOCH_CASES))
def test_epoch_kernels_per_rank_equal_the_epoch_restatement(name):
    """nrhip_route_epoch and nrhip_route_epoch_owner_keys, called as RowRouter._build_tables calls them; the gap of a
    short last slot keeps the sentinel"""
    import torch
    from neurec_amd import engine as E
    U, I, W, B, streams = R.make_epoch_case(name)
    lay, ep = R.Layout(U, I, W), R.restate_epoch(U, I, W, B, streams)
    for r, w in enumerate(ep):
        nb, n = w["nb"], len(streams[r][0])
        users, pos, neg = (_i32(x) for x in streams[r])
        slots = 3 * nb * B
        keys, packed = _out((slots,), torch.int64), _out((slots, 2), torch.int32)
        order, inv, counts = _out((slots,), torch.int32), _out((slots,), torch.int32), _out((nb * W,), torch.int32, 99)
        seg_off, seg_len = _dev(np.arange(nb) * 3 * B, np.int64), _i32(3 * w["sizes"][:, r])
        E.call("nrhip_route_epoch", E._ptr(users), E._ptr(pos), E._ptr(neg), n, B, U, lay.bu, lay.bi, R.CODE, W,
               E._ptr(keys), E._ptr(packed), E._ptr(order), E._ptr(inv), E._ptr(counts), E._ptr(seg_off),
               E._ptr(seg_len), E._stream())
        np.testing.assert_array_equal(_host(keys), w["keys"], err_msg="keys of rank %d" % r)
        for got, f in ((packed, "packed"), (order, "order"), (inv, "inv")):
            want = np.where(w[f] == R.FILL, SENT, w[f])
            assert (want == SENT).any() == (w["sizes"][-1, r] < B)        # the short slot has a gap to leave alone
            np.testing.assert_array_equal(_host(got), want, err_msg="%s of rank %d" % (f, r))
        np.testing.assert_array_equal(_host(counts).reshape(nb, W), w["send"], err_msg="counts of rank %d" % r)
        # the owner's side of the same epoch
        m, stride = len(w["asked"]), w["iop_stride"]
        okeys, iop = _out((m + 2,), torch.int64), _out((nb * stride,), torch.int32)
        rows, codes, batch_of = _i32(w["asked"]), _i32(w["asked_code"]), _i32(w["batch_of"])
        asked_off, asked_len = _dev(w["asked_off"], np.int64), _i32(np.diff(w["asked_off"]))
        recv_prefix, size_off, glen = _i32(w["recv_prefix"]), _i32(w["size_off"]), _i32(w["glen"])
        E.call("nrhip_route_epoch_owner_keys", E._ptr(rows), E._ptr(codes), E._ptr(batch_of), m, E._ptr(asked_off),
               E._ptr(asked_len), nb, w["max_asked"], E._ptr(recv_prefix), E._ptr(size_off), E._ptr(glen), W, R.CODE,
               stride, E._ptr(okeys), E._ptr(iop), E._stream())
        np.testing.assert_array_equal(_host(okeys), np.concatenate([w["okeys"], [SENT, SENT]]),
                                      err_msg="owner keys of rank %d" % r)
        want = np.where(w["index_of_pos"] == R.FILL, SENT, w["index_of_pos"]).reshape(-1)
        np.testing.assert_array_equal(_host(iop), want, err_msg="index_of_pos of rank %d" % r)


# ------------------------------------------------------------------------ RowRouter at W > 1 through a scripted comm
def _scripted(W, rank, part, max_batch):
    """a RowRouter whose communicator and count exchange read from a script written by the restatement: every send is
    asserted to be what the restatement says this rank sends, every receive is what it says arrives.  Nothing here
    calls torch.distributed."""
    import torch
    from neurec_amd.sharded import RowRouter

    class Comm:
        live, backend = True, "scripted"

        def __init__(self):
            self.world, self.rank, self.script, self.global_max = W, rank, [], None

        def all_to_all_rows(self, send, send_counts, recv_counts=None):
            want_send, want_sc, recv, want_rc = self.script.pop(0)
            assert [int(c) for c in send_counts] == [int(c) for c in want_sc]
            assert recv_counts is not None and [int(c) for c in recv_counts] == [int(c) for c in want_rc]
            np.testing.assert_array_equal(_host(send), want_send)
            return _i32(recv).reshape(-1, 2), [int(c) for c in want_rc]

        def max_float(self, x):
            assert self.global_max is not None and x <= self.global_max
            return float(self.global_max)

    class Router(RowRouter):
        exchange = None

        def _exchange_counts(self, send, sizes):
            want_send, want_sizes, recv, all_sizes = self.exchange.pop(0)
            np.testing.assert_array_equal(_host(send), want_send)
            np.testing.assert_array_equal(_host(sizes), want_sizes)
            return (_dev(recv, np.int64).to(send.device).reshape(send.shape),
                    _dev(all_sizes, np.int64).to(send.device).reshape(send.shape))

    comm = Comm()
    router = Router(comm, part, max_batch)
    router.exchange = []
    return router, comm


def _check_route(rt, w, where):
    for f in ("order", "inv", "asked", "asked_code", "recv_prefix", "size_off"):
        np.testing.assert_array_equal(_host(getattr(rt, f)), w[f], err_msg="%s %s" % (f, where))
    assert [int(c) for c in rt.send_counts] == w["send_counts"].tolist(), where
    assert [int(c) for c in rt.recv_counts] == w["recv_counts"].tolist(), where
    assert rt.G == w["G"], where


def _check_keys(keys, iop, w, where):
    np.testing.assert_array_equal(_host(keys), w["okeys"], err_msg="keys %s" % where)
    assert iop.numel() >= 3 * w["G"]
    np.testing.assert_array_equal(_host(iop)[w["gpos"]], np.arange(len(w["gpos"])), err_msg="index_of_pos %s" % where)


def _script_request(router, comm, w, sizes, counted):
    if counted:
        router.exchange.append((w["send_counts"][None, :], [w["B"]], w["recv_counts"][None, :],
                                np.asarray(sizes)[None, :]))
    comm.script.append((w["packed"], w["send_counts"], _pairs(w["asked"], w["asked_code"]), w["recv_counts"]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_row_router_request_and_ordered_keys_on_every_rank(name):
    """`request` counted on the spot (no plan) + `ordered_keys`, every field of the Route; each rank twice on its
    router, and a rank with an empty batch right after a full batch went through the same router"""
    from neurec_amd import parallel
    U, I, W, batches = R.make_case(name)
    res = R.restate(U, I, W, batches)
    part = parallel.BipartitePartition(U, I, W)
    sizes = [len(b[0]) for b in batches]
    full = [r for r in range(W) if sizes[r] > 0]
    for r in range(W):
        router, comm = _scripted(W, r, part, max(sizes))
        turns = ([full[0]] if sizes[r] == 0 else []) + [r, r]
        for who in turns:
            _script_request(router, comm, res[who], sizes, counted=True)
            rt = router.request(*(_i32(x) for x in batches[who]), U)
            assert not comm.script and not router.exchange
            where = "(rank %d on the router of rank %d)" % (who, r)
            _check_route(rt, res[who], where)
            assert rt.keys is None
            _check_keys(*router.ordered_keys(rt), res[who], where)


@pytest.mark.parametrize("tables", [True, False], ids=["tables", "counts_only"])
@pytest.mark.parametrize("name", sorted(EPOCH_CASES))
def test_row_router_plan_epoch_on_every_rank(name, tables):
    """plan_epoch down to planned_route (tables: the destination-major / source-major arithmetic of _build_tables), or
    with the counts alone and `request` + `ordered_keys` per batch; every field, per rank and per batch"""
    from neurec_amd import parallel
    U, I, W, B, streams = R.make_epoch_case(name)
    ep = R.restate_epoch(U, I, W, B, streams)
    nb = ep[0]["nb"]
    per = [R.restate(U, I, W, [tuple(c[k * B:(k + 1) * B] for c in s) for s in streams]) for k in range(nb)]
    part = parallel.BipartitePartition(U, I, W)
    for r, e in enumerate(ep):
        router, comm = _scripted(W, r, part, B)
        comm.global_max = e["max_asked"]
        classes = [_i32(x) for x in streams[r]]
        router.exchange.append((e["send"], e["sizes"][:, r], e["recv"], e["sizes"]))
        if tables:
            comm.script.append((e["to_owners"], e["tot_send"], e["from_sources"], e["tot_recv"]))
        router.plan_epoch(classes, (0, U, U), B, tables=tables)
        assert not comm.script and not router.exchange
        assert (router._tables is not None) == tables
        for k in range(nb):
            p, where = per[k][r], "(rank %d, batch %d)" % (r, k)
            Bk = p["B"]
            assert router.epoch_counts(k, Bk + 1) is None                  # a batch of another length was not planned
            if tables:
                rt = router.planned_route(k, Bk)
                assert rt is not None and rt.keys is not None and rt.index_of_pos.numel() == 3 * p["G"]
            else:
                assert router.planned_route(k, Bk) is None
                planned = router.epoch_counts(k, Bk)
                assert planned is not None
                _script_request(router, comm, p, None, counted=False)
                rt = router.request(*(c[k * B:k * B + Bk].contiguous() for c in classes), U, planned)
                assert not comm.script
            _check_route(rt, p, where)
            _check_keys(*router.ordered_keys(rt), p, where)
        assert router.epoch_counts(nb, B) is None and router.planned_route(nb, B) is None


def test_a_batch_that_asks_an_owner_for_more_than_one_sorting_workgroup_is_not_planned():
    """W = 2, B = 5461, every id owned by rank 0: 3·B = 16383 fits, the 32766 rows rank 0 is asked for do not —
    planned_route is None on EVERY rank (rank 1 is asked for nothing and must decide the same), the counts stay valid"""
    from neurec_amd import parallel
    U, I, W, B = 64, 64, 2, 5461
    rng = np.random.RandomState(5)
    streams = [R._draw(rng, U, I, W, B, 0) for _ in range(W)]
    ep = R.restate_epoch(U, I, W, B, streams)
    assert 3 * B <= 16384 < ep[0]["max_asked"] == 6 * B
    part = parallel.BipartitePartition(U, I, W)
    for r, e in enumerate(ep):
        router, comm = _scripted(W, r, part, B)
        comm.global_max = e["max_asked"]
        router.exchange.append((e["send"], e["sizes"][:, r], e["recv"], e["sizes"]))
        router.plan_epoch([_i32(x) for x in streams[r]], (0, U, U), B)     # an all-to-all here would find no script
        assert router._tables is None and router.planned_route(0, B) is None
        send_counts, recv_counts, sizes, recv_prefix, size_off = router.epoch_counts(0, B)
        assert send_counts == e["send"][0].tolist() == [3 * B, 0]
        assert recv_counts == e["recv"][0].tolist() == ([3 * B, 3 * B] if r == 0 else [0, 0])
        assert sizes == [B, B]
        np.testing.assert_array_equal(_host(recv_prefix), e["recv_prefix"][0])
        np.testing.assert_array_equal(_host(size_off), [0, B])


# ------------------------------------------------------------------------------------ the sums the routing exists for
def _duplicates(nodes, rank_of):
    """(a node looked up twice by one rank, a node looked up by two ranks)?"""
    within = any(np.unique(nodes[rank_of == r], return_counts=True)[1].max(initial=0) > 1 for r in np.unique(rank_of))
    pairs = np.unique(np.stack([nodes, rank_of], 1), axis=0)
    across = np.unique(pairs[:, 0], return_counts=True)[1].max(initial=0) > 1
    return bool(within), bool(across)


@pytest.mark.parametrize("d", [20, 64])
@pytest.mark.parametrize("name", ["uneven_w4", "duplicates_w8", "all_to_rank1"])
def test_owner_sums_reassembled_are_the_ordered_sum_over_the_concatenated_batch(name, d):
    """one random fp32 gradient row per occurrence of the global batch, delivered as the engine delivers them (gathered
    by `order`, exchanged), summed per owner by nrhip_rows_sum_sorted along the routed keys: the [U + I][d] table put
    together from the owners' blocks is BIT-identical to np.add.at over the concatenated batch in position order"""
    import torch
    from neurec_amd import engine as E
    U, I, W, batches = R.make_case(name)
    lay, res = R.Layout(U, I, W), R.restate(U, I, W, batches)
    G = res[0]["G"]
    rng = np.random.RandomState(d)
    grads = [rng.randn(3 * len(b[0]), d).astype(np.float32) for b in batches]      # row p = class · B + b of rank r
    nodes, rank_of, rows = np.empty(3 * G, np.int64), np.empty(3 * G, np.int64), np.empty((3 * G, d), np.float32)
    for r, (users, pos, neg) in enumerate(batches):
        B = len(users)
        for c, ids in enumerate((users.astype(np.int64), U + pos.astype(np.int64), U + neg.astype(np.int64))):
            at = c * G + res[r]["size_off"][r] + np.arange(B)
            nodes[at], rank_of[at], rows[at] = ids, r, grads[r][c * B:(c + 1) * B]
    want = np.zeros((U + I, d), np.float32)
    np.add.at(want, nodes, rows)                                                    # position order, fp32
    assert _duplicates(nodes, rank_of) == (True, True)
    routed = [grads[r][res[r]["order"]] for r in range(W)]
    table = np.zeros((U + I, d), np.float32)
    for t, w in enumerate(res):
        parts = []
        for s in range(W):
            lo = int(res[s]["send_counts"][:t].sum())
            parts.append(routed[s][lo:lo + int(res[s]["send_counts"][t])])
        mine = np.concatenate(parts).reshape(-1, d)
        m = len(w["asked"])
        assert mine.shape[0] == m
        keys = torch.empty(m, dtype=torch.int64, device="cuda")
        iop = _out((max(3 * G, 1),), torch.int32)
        E.route_owner_keys(_i32(w["asked"]), _i32(w["asked_code"]), _i32(w["recv_prefix"]), _i32(w["size_off"]), W, G,
                           R.CODE, keys, iop)
        _check_keys(keys, iop, w, "(owner %d)" % t)              # before they address anything
        assert m == 0 or (0 <= _host(keys) >> 32).all() and (_host(keys) >> 32).max() < lay.b
        block = torch.zeros((lay.b, d), dtype=torch.float32, device="cuda")
        E.rows_sum_sorted(keys, iop, _dev(mine, np.float32), block)
        block = block.cpu().numpy()
        held = lay.node_at[t] >= 0
        assert not block[~held].any()                            # padding rows of the block receive nothing
        table[lay.node_at[t][held]] = block[held]
    np.testing.assert_array_equal(table.view(np.uint32), want.view(np.uint32))
