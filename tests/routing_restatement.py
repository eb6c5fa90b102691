"""A plain numpy statement of the routing of the row-sharded engines (neurec_amd/sharded.py: RowRouter;
neurec_amd/csrc/route.hip), for any number of ranks W, on one host.  No torch, no GPU.

What is stated (MF.py:57-58 / LightGCN.py:99-104: tf.nn.embedding_lookup of 3·B rows per rank, the gradient rows added by
unsorted_segment_sum over the CONCATENATED batch of all ranks):
  * the table is cut into per-rank blocks: rank r holds its users, then its items (`Layout`, written as the list of
    nodes every rank holds, not as the division the kernels use);
  * a rank's 3·B requests (users, positives, negatives) travel grouped by owner, inside an owner in request order, each
    as a pair (row in the owner's block, occurrence code = class · CODE + position in the rank's batch);
  * an owner receives the pairs source rank by source rank and gives every occurrence its position in the global batch
    — class-major, then source rank, then position in that rank's batch — which is the order its gradient rows are added
    in: keys (row << 32 | global position), sorted, and index_of_pos[global position] = place among the received pairs.
`restate` does this for one batch per rank by walking ranks and owners; `restate_epoch` does it for whole per-rank
streams cut into batches of B by sorting ONE table of all requests of all ranks and batches, in the layouts
RowRouter._build_tables keeps.  The two are written apart on purpose: tests/test_routing_cpu.py compares them."""
import numpy as np

CODE = 1 << 24          # RowRouter.CODE
FILL = -7               # what an entry nobody writes holds in the arrays returned here


class Layout:
    """who holds which node: rank r's block = users [r·bu, (r+1)·bu) then items [r·bi, (r+1)·bi), clipped to the
    tables' ends (the last ranks may hold fewer rows, or none), bu = ceil(U / W), bi = ceil(I / W)"""

    def __init__(self, U, I, W):
        self.U, self.I, self.W = int(U), int(I), int(W)
        self.bu, self.bi = -(-self.U // self.W), -(-self.I // self.W)
        self.b = self.bu + self.bi
        self.owner = np.full(self.U + self.I, -1, np.int64)
        self.local = np.full(self.U + self.I, -1, np.int64)
        self.node_at = np.full((self.W, self.b), -1, np.int64)           # [rank][block row] -> node, -1 = padding
        for r in range(self.W):
            held = list(range(min(r * self.bu, self.U), min((r + 1) * self.bu, self.U)))
            for row, u in enumerate(held):
                self.owner[u], self.local[u], self.node_at[r, row] = r, row, u
            held = list(range(min(r * self.bi, self.I), min((r + 1) * self.bi, self.I)))
            for row, i in enumerate(held):
                self.owner[self.U + i], self.local[self.U + i], self.node_at[r, self.bu + row] = r, self.bu + row, self.U + i
        assert (self.owner >= 0).all()


def _i64(a):
    return np.asarray(a, dtype=np.int64).reshape(-1)


def restate(U, I, W, batches):
    """batches: one (users, pos, neg) per rank, each of any length, 0 included.  -> one dict per rank:
      order, inv [3B]         order[i] = the request (class · B + b) that travels at place i; inv = its inverse
      packed [3B][2]          (row in the owner's block, occurrence code) at place i
      keys [3B]               (owner << 32 | request), ascending: the scratch nrhip_route_batch leaves behind
      send_counts [W]         requests per owner
      asked, asked_code [m]   what this rank is asked for, source rank by source rank; recv_counts [W]
      recv_prefix [W + 1], size_off [W], G      offsets of the sources in `asked`, of the ranks' batches in the global
                              batch, and the global batch length
      gpos [m]                global position of every received occurrence
      okeys [m]               (row << 32 | gpos), ascending
      index_of_pos [3G]       index_of_pos[gpos[i]] = i; FILL at the positions other owners hold"""
    lay = Layout(U, I, W)
    assert len(batches) == W
    sizes = [len(b[0]) for b in batches]
    G = int(sum(sizes))
    size_off = [int(sum(sizes[:r])) for r in range(W)]
    out = []
    for r, (users, pos, neg) in enumerate(batches):
        B = sizes[r]
        assert len(pos) == B and len(neg) == B
        node = np.concatenate([_i64(users), U + _i64(pos), U + _i64(neg)])
        code = np.concatenate([c * CODE + np.arange(B, dtype=np.int64) for c in range(3)])
        own = lay.owner[node]
        order = np.argsort(own, kind="stable")              # grouped by owner, request order kept inside an owner
        inv = np.empty(3 * B, np.int64)
        inv[order] = np.arange(3 * B)
        out.append(dict(B=B, order=order, inv=inv, packed=np.stack([lay.local[node][order], code[order]], 1),
                        keys=(own[order] << 32) | order, send_counts=np.bincount(own, minlength=W).astype(np.int64),
                        G=G, size_off=np.array(size_off, np.int64)))
    for t in range(W):                                      # the exchange: owner t hears from every source in rank order
        parts, recv = [], []
        for s in range(W):
            lo = int(out[s]["send_counts"][:t].sum())
            hi = lo + int(out[s]["send_counts"][t])
            parts.append(out[s]["packed"][lo:hi])
            recv.append(hi - lo)
        got = np.concatenate(parts).reshape(-1, 2)
        m = got.shape[0]
        src = np.repeat(np.arange(W), recv)
        cls, b = got[:, 1] // CODE, got[:, 1] % CODE
        gpos = cls * G + np.array(size_off, np.int64)[src] + b
        iop = np.full(3 * G, FILL, np.int64)
        iop[gpos] = np.arange(m)
        out[t].update(asked=got[:, 0].copy(), asked_code=got[:, 1].copy(), recv_counts=np.array(recv, np.int64),
                      recv_prefix=np.concatenate([[0], np.cumsum(recv)]).astype(np.int64), gpos=gpos,
                      okeys=np.sort((got[:, 0] << 32) | gpos), index_of_pos=iop)
    return out


def restate_epoch(U, I, W, B, streams):
    """streams: one (users, pos, neg) per rank, cut into batches of B (the last may be short; the number of batches is
    the same on every rank, the last batches' lengths need not be).  -> one dict per rank, nb batches:
      order, inv [3·nb·B], packed [3·nb·B][2], keys [3·nb·B]    batch k in slot [3·B·k, 3·B·(k+1)), a short batch's
                              requests at the slot's start; FILL in the gap (keys: -1, all bits set)
      send [nb][W], recv [nb][W], sizes [nb][W] (every rank's batch lengths), glen [nb], recv_prefix [nb][W + 1],
      size_off [nb][W]
      asked, asked_code [m]   the received pairs laid out [batch][source rank]; asked_off [nb + 1]; batch_of [m]
      okeys [m]               per batch ascending, batch k at asked_off[k]
      iop_stride = 3 · max glen; index_of_pos [nb][iop_stride] (FILL where this owner holds nothing)
      to_owners [3n][2] / tot_send [W]      the epoch's one all-to-all as this rank sends it: destination-major, batches
                              in order inside a destination;  from_sources [m][2] / tot_recv [W]: as it arrives,
                              source-major, batches in order inside a source
      max_asked               the most any owner is asked for in one batch (the same number on every rank)"""
    lay = Layout(U, I, W)
    lens = [len(s[0]) for s in streams]
    nb = -(-lens[0] // B)
    assert all(-(-n // B) == nb for n in lens) and nb >= 1
    sizes = np.array([[min(B, n - k * B) for n in lens] for k in range(nb)], np.int64)        # [nb][W]
    glen = sizes.sum(1)
    size_off = np.cumsum(sizes, 1) - sizes
    # one table of every request of every rank: source, batch, class, place in the batch, node
    src, bat, cls, plc, node = [], [], [], [], []
    for s, (users, pos, neg) in enumerate(streams):
        j = np.arange(lens[s], dtype=np.int64)
        for c, ids in enumerate((_i64(users), U + _i64(pos), U + _i64(neg))):
            src.append(np.full(lens[s], s, np.int64)), bat.append(j // B), cls.append(np.full(lens[s], c, np.int64))
            plc.append(j % B), node.append(ids)
    src, bat, cls, plc, node = (np.concatenate(x) for x in (src, bat, cls, plc, node))
    req = cls * sizes[bat, src] + plc                       # the request's number inside its (rank, batch)
    own, row = lay.owner[node], lay.local[node]
    code = cls * CODE + plc
    gpos = cls * glen[bat] + size_off[bat, src] + plc
    key = (row << 32) | gpos
    stride = 3 * int(glen.max())
    asked_per = np.zeros((W, nb), np.int64)
    np.add.at(asked_per, (own, bat), 1)
    out = []
    for r in range(W):
        mine = np.flatnonzero(src == r)
        mine = mine[np.lexsort((req[mine], own[mine], bat[mine]))]          # by batch, then owner, then request
        place = np.arange(len(mine)) - np.searchsorted(bat[mine], bat[mine], side="left")     # place inside the batch
        slot = 3 * B * bat[mine] + place
        order, inv, keys = (np.full(3 * nb * B, FILL, np.int64) for _ in range(3))
        keys[:] = -1
        packed = np.full((3 * nb * B, 2), FILL, np.int64)
        order[slot], inv[3 * B * bat[mine] + req[mine]] = req[mine], place
        packed[slot, 0], packed[slot, 1], keys[slot] = row[mine], code[mine], (own[mine] << 32) | req[mine]
        send = np.zeros((nb, W), np.int64)
        np.add.at(send, (bat[mine], own[mine]), 1)
        away = mine[np.lexsort((req[mine], bat[mine], own[mine]))]          # by owner, then batch, then request
        # the owner's side
        got = np.flatnonzero(own == r)
        got = got[np.lexsort((req[got], src[got], bat[got]))]               # by batch, then source, then request
        recv = np.zeros((nb, W), np.int64)
        np.add.at(recv, (bat[got], src[got]), 1)
        per = recv.sum(1)
        asked_off = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        within = np.arange(len(got)) - asked_off[bat[got]]
        iop = np.full((nb, stride), FILL, np.int64)
        iop[bat[got], gpos[got]] = within
        srt = got[np.lexsort((key[got], bat[got]))]                         # by batch, then key
        arrive = got[np.lexsort((req[got], bat[got], src[got]))]            # by source, then batch, then request
        out.append(dict(
            nb=nb, B=B, order=order, inv=inv, packed=packed, keys=keys, send=send, recv=recv, sizes=sizes, glen=glen,
            recv_prefix=np.concatenate([np.zeros((nb, 1), np.int64), np.cumsum(recv, 1)], 1), size_off=size_off,
            asked=row[got], asked_code=code[got], asked_off=asked_off, batch_of=bat[got], okeys=key[srt],
            iop_stride=stride, index_of_pos=iop, to_owners=np.stack([row[away], code[away]], 1),
            tot_send=send.sum(0), from_sources=np.stack([row[arrive], code[arrive]], 1), tot_recv=recv.sum(0),
            max_asked=int(asked_per.max())))
    return out


# ---- the shapes the tests share: (U, I, W, per-rank batch lengths, rank that owns every id or None)
CASES = {
    "uneven_w4": (10, 7, 4, [5, 0, 3, 1], None),
    "three_empty_ranks": (5, 3, 4, [0, 0, 1, 0], None),          # rank 3 owns no user and no item
    "one_row_w5": (1, 1, 5, [2, 0, 0, 0, 7], None),
    "w3_unequal": (500, 700, 3, [96, 17, 1], None),
    "duplicates_w8": (37, 53, 8, [33] * 8, None),                # few rows: long runs of duplicates
    "block_edge_w2": (300, 200, 2, [257, 255], None),            # 3·B straddles a 256-thread block
    "all_to_rank1": (64, 64, 2, [40, 25], 1),                    # rank 0 is asked for nothing
}
# epoch streams: (U, I, W, B, full batches before the last, per-rank last-batch lengths)
EPOCH_CASES = {
    "w3_short_last": (500, 700, 3, 96, 5, [17, 1, 96]),
    "uneven_w4": (10, 7, 4, 96, 5, [17, 1, 96, 50]),
}


def _draw(rng, U, I, W, n, only):
    """n triplets; only = r: every id from the rows rank r holds"""
    lay = Layout(U, I, W)
    ulo, uhi, ilo, ihi = 0, U, 0, I
    if only is not None:
        ulo, uhi = min(only * lay.bu, U), min((only + 1) * lay.bu, U)
        ilo, ihi = min(only * lay.bi, I), min((only + 1) * lay.bi, I)
    return tuple(rng.randint(lo, hi, n).astype(np.int32) for lo, hi in ((ulo, uhi), (ilo, ihi), (ilo, ihi)))


def make_case(name):
    """-> (U, I, W, [one (users, pos, neg) int32 batch per rank]); the same numbers on every call"""
    U, I, W, lens, only = CASES[name]
    rng = np.random.RandomState(sorted(CASES).index(name) + 100)
    return U, I, W, [_draw(rng, U, I, W, n, only) for n in lens]


def make_epoch_case(name):
    """-> (U, I, W, B, [one (users, pos, neg) int32 stream per rank])"""
    U, I, W, B, full, last = EPOCH_CASES[name]
    rng = np.random.RandomState(sorted(EPOCH_CASES).index(name) + 200)
    return U, I, W, B, [_draw(rng, U, I, W, full * B + n, None) for n in last]
