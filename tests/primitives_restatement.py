"""A numpy restatement of the shared training primitives (csrc/adam.hip: the row and dense optimisers of
util/learner.py; csrc/bpr.hip: the general MF gradients and the ordered row sums) and the inputs the primitive tests
feed them.  Every function works in the dtype of its arrays: with float32 arrays it performs the operations in the order
the kernel comments document, one rounding per operation, and is the bit-exact expectation; with float64 arrays the same
function is the high-precision reference.  Hyper-parameters are rounded to float32 first in both widths, as the C ABI
receives them, so both widths restate the same operation on the same numbers.  The MF gradients are
oracle.train.mf_general_loss_and_grads in both widths.  Checked on the host in test_primitives_cpu.py; the inputs are
built once per case and handed out read-only."""
import functools

import numpy as np

from oracle import train

# (kind, hyper1, hyper2, eps): learner.py:2-16 as TF-1.12 runs them, and RMSProp with a momentum no engine passes
OPTIMIZERS = [("gd", 0.0, 0.0, 0.0), ("adagrad", 0.0, 0.0, 0.0), ("rmsprop", 0.9, 0.0, 1e-10),
              ("rmsprop", 0.9, 0.5, 1e-10), ("momentum", 0.9, 0.0, 0.0)]


def _hyper(dt, *xs):
    return [dt(np.float32(x)) for x in xs]


# ------------------------------------------------------------------ the optimisers
def optimizer_rows(kind, var, s0, s1, grad, flag, lr, h1=0.0, h2=0.0, eps=0.0):
    """nrhip_optimizer_rows_tf in place: the flagged rows move, their gradient rows and flags are cleared
         gd        var -= lr*g
         adagrad   a += g*g;                     var -= (lr*g) * (1/sqrt(a))
         rmsprop   ms = ms*rho + (g*g)*(1-rho);  mom = mom*momentum + ((1/sqrt(ms+eps))*lr)*g;  var -= mom
         momentum  a = a*momentum + g;           var -= a*lr"""
    dt = var.dtype.type
    one = dt(1)
    lr, h1, h2, eps = _hyper(dt, lr, h1, h2, eps)
    r = np.flatnonzero(flag)
    g = grad[r]
    if kind == "gd":
        var[r] = var[r] - lr * g
    elif kind == "adagrad":
        s0[r] = s0[r] + g * g
        var[r] = var[r] - (lr * g) * (one / np.sqrt(s0[r]))
    elif kind == "rmsprop":
        s0[r] = s0[r] * h1 + (g * g) * (one - h1)
        s1[r] = s1[r] * h2 + ((one / np.sqrt(s0[r] + eps)) * lr) * g
        var[r] = var[r] - s1[r]
    elif kind == "momentum":
        s0[r] = s0[r] * h1 + g
        var[r] = var[r] - s0[r] * lr
    else:
        raise ValueError(kind)
    grad[r] = 0
    flag[r] = 0


def optimizer_dense(kind, var, s0, s1, grad, lr, h1=0.0, h2=0.0, eps=0.0, clear_grad=False):
    """nrhip_optimizer_dense_tf in place (TF-1.12's Apply* kernels: every element moves)
         gd        var -= g*lr
         adagrad   a += g*g;                     var -= (g*lr) * (1/sqrt(a))
         rmsprop   ms += (g*g - ms)*(1-rho);     mom = mom*momentum + (g*lr)/sqrt(eps+ms);  var -= mom
         momentum  a = a*momentum + g;           var -= a*lr"""
    dt = var.dtype.type
    one = dt(1)
    lr, h1, h2, eps = _hyper(dt, lr, h1, h2, eps)
    g = grad
    if kind == "gd":
        var[...] = var - g * lr
    elif kind == "adagrad":
        s0[...] = s0 + g * g
        var[...] = var - (g * lr) * (one / np.sqrt(s0))
    elif kind == "rmsprop":
        s0[...] = s0 + (g * g - s0) * (one - h1)
        s1[...] = s1 * h2 + (g * lr) / np.sqrt(eps + s0)
        var[...] = var - s1
    elif kind == "momentum":
        s0[...] = s0 * h1 + g
        var[...] = var - s0 * lr
    else:
        raise ValueError(kind)
    if clear_grad:
        grad[...] = 0


def optimizer_inputs(kind, shape, seed):
    """(var, slot0, slot1) in float32: generic values (slot0 positive: it is a sum of squares under two of the kinds)"""
    rs = np.random.RandomState(seed)
    f = lambda a: np.asarray(a, np.float32)
    return f(rs.randn(*shape)), f(0.1 + rs.rand(*shape)), f(0.1 * rs.randn(*shape))


def flag_pattern(pattern, n_rows, rs):
    if pattern == "some":
        return (rs.rand(n_rows) < 0.4).astype(np.uint8)
    return np.full(n_rows, {"none": 0, "all": 1}[pattern], np.uint8)


# ------------------------------------------------------------------ ordered row sums
def rows_sum_sorted(keys, index_of_pos, src, dst):
    """nrhip_rows_sum_sorted in place: per run of one row in the sorted keys (row << 32 | position) the source rows
    src[index_of_pos[position]] are added one at a time in key order (the first stored) and the sum stored into
    dst[row]; the other rows of dst stay"""
    keys = np.asarray(keys, np.int64)
    k = 0
    while k < len(keys):
        row = keys[k] >> 32
        acc = src[index_of_pos[keys[k] & 0xffffffff]].copy()
        k += 1
        while k < len(keys) and keys[k] >> 32 == row:
            acc = acc + src[index_of_pos[keys[k] & 0xffffffff]]
            k += 1
        dst[row] = acc


ROWSUM_DIMS = (1, 64, 65, 128, 129, 256)
ROWSUM_NS = (1, 4, 5, 300)
ROWSUM_ROWS = 40            # rows of the destination
ROWSUM_CANARY = -3.5


@functools.lru_cache(maxsize=None)
def rowsum_case(d, n):
    """sorted keys, index_of_pos (a random permutation), two wide sources ([n][d + 3]) and the destination rows with
    keys.  n = 1: one key; n = 4: a run of three and a run of one (one workgroup of four waves); n = 5: a run of one,
    then a run of four that leaves the first workgroup; n = 300: a run of 70, a run of exactly 1, the rest random"""
    rs = np.random.RandomState(7 * d + n)
    rows = {1: [6], 4: [5, 5, 5, 9], 5: [2, 5, 5, 5, 5]}.get(n)
    if rows is None:
        others = np.setdiff1d(np.arange(ROWSUM_ROWS), [3, 17, 39])
        rows = [3] * 70 + [17] + rs.choice(others, n - 71).tolist()
    rows = np.asarray(rows, np.int64)
    keys = np.sort((rows << 32) | rs.permutation(n).astype(np.int64))
    out = {"keys": keys, "index_of_pos": rs.permutation(n).astype(np.int32),
           "src_a": rs.randn(n, d + 3).astype(np.float32), "src_b": rs.randn(n, d + 3).astype(np.float32),
           "rows": np.unique(rows)}
    for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
        for s in ("a", "b"):
            dst = np.full((ROWSUM_ROWS, d), ROWSUM_CANARY, dt)
            rows_sum_sorted(keys, out["index_of_pos"], out["src_" + s][:, :d].astype(dt), dst)
            out["%s_%s" % (tag, s)] = dst
    return _frozen(out)


def run_lengths(keys):
    """[(row, first sorted position, length)] of the runs of sorted keys"""
    rows = np.asarray(keys, np.int64) >> 32
    starts = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
    return [(int(rows[s]), int(s), int(e - s)) for s, e in zip(starts, np.r_[starts[1:], len(rows)])]


# ------------------------------------------------------------------ the MF gradients
MF_USERS, MF_ITEMS = 23, 31
MF_REG = 0.01
MF_DIMS = (1, 20, 64, 65, 128, 129, 256)           # both sides of the 64- and 128-column layouts, and the widest
MF_BATCHES = (1, 5, 6, 33, 71)                     # 5: 15 occurrences, inside one 16-occurrence workgroup; 6: 18
MF_LOSSES = [(True, "bpr"), (True, "hinge"), (True, "square"), (False, "cross_entropy"), (False, "square")]
MF_CONSTRUCTED = ("run16", "run32", "run40", "item_both")
MF_CONSTRUCTED_DIMS = (20, 65, 129)                # one, two and four columns per lane
OCC_PER_WORKGROUP = 16                             # csrc/bpr.hip: kOccWaves
RUN40_USER, BOTH_ITEM = 11, 7


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def mf_tables(d):
    """entries of size d^(-1/4): the logit differences are O(1), so the hinge is cut for some triplets and not for
    others and no sigmoid saturates"""
    rs = np.random.RandomState(100 + d)
    s = float(d) ** -0.25
    P, Q = (s * rs.randn(MF_USERS, d)).astype(np.float32), (s * rs.randn(MF_ITEMS, d)).astype(np.float32)
    P.setflags(write=False)
    Q.setflags(write=False)
    return P, Q


def constructed_batch(name):
    """64 slots (users, items, negatives) with one long run in the sorted occurrence list:
         run16      user 0 (the lowest id) in exactly 16 slots: its run is workgroup 0, exactly
         run32      user 0 in exactly 32 slots: workgroups 0 and 1, exactly
         run40      user 11 in 40 slots behind 5 slots of lower users: sorted positions 5 .. 44, workgroup 1 in the middle
         item_both  item 7 the positive of 20 slots, the negative of 20 others and both of slot 40"""
    rs = np.random.RandomState(MF_CONSTRUCTED.index(name))
    B = 64
    users = rs.randint(1, MF_USERS, B)
    items, negs = rs.randint(0, MF_ITEMS, B), rs.randint(0, MF_ITEMS, B)
    order = rs.permutation(B)
    if name in ("run16", "run32"):
        users[order[:int(name[3:])]] = 0
    elif name == "run40":
        users[order[:40]] = RUN40_USER
        users[order[40:45]] = rs.randint(0, RUN40_USER, 5)
        users[order[45:]] = rs.randint(RUN40_USER + 1, MF_USERS, B - 45)
    else:
        away = np.setdiff1d(np.arange(MF_ITEMS), [BOTH_ITEM])
        items, negs = rs.choice(away, B), rs.choice(away, B)
        items[order[:20]] = BOTH_ITEM
        negs[order[20:40]] = BOTH_ITEM
        items[order[40]] = negs[order[40]] = BOTH_ITEM
    return users.astype(np.int32), items.astype(np.int32), negs.astype(np.int32)


def host_plan(users, items, third, n_users):
    """the batch plan of csrc/bpr.hip sorted on the host: keys (row << 32 | class * B + slot), rows = user id or
    n_users + item id, class 0 the users, 1 the items, 2 the negatives (pairwise only: third is not None)"""
    B = len(users)
    rows = [np.asarray(users, np.int64), n_users + np.asarray(items, np.int64)]
    if third is not None:
        rows.append(n_users + np.asarray(third, np.int64))
    return np.sort(np.concatenate([(r << 32) | (c * B + np.arange(B)) for c, r in enumerate(rows)]))


def mf_gradients(P, Q, users, items, third, pairwise, kind, dtype, reg=MF_REG):
    """(loss2[0], loss2[1], dP, dQ) of oracle.train.mf_general_loss_and_grads in `dtype`; reg as the ABI receives it"""
    third = third if pairwise else np.asarray(third, dtype)
    return train.mf_general_loss_and_grads(P.astype(dtype), Q.astype(dtype), users, items, third,
                                           float(np.float32(reg)), pairwise, kind)


@functools.lru_cache(maxsize=None)
def mf_case(pairwise, kind, d, batch):
    """inputs and both restatements of one case; batch: a size of MF_BATCHES (random slots) or a name of MF_CONSTRUCTED"""
    P, Q = mf_tables(d)
    if isinstance(batch, str):
        users, items, negs = constructed_batch(batch)
    else:
        rs = np.random.RandomState(1000 * d + batch)
        users, items, negs = (rs.randint(0, hi, batch).astype(np.int32) for hi in (MF_USERS, MF_ITEMS, MF_ITEMS))
    labels = (np.random.RandomState(len(users)).rand(len(users)) < 0.4).astype(np.float32)
    third = negs if pairwise else labels
    out = {"P": P, "Q": Q, "users": users, "items": items, "third": third,
           "plan": host_plan(users, items, negs if pairwise else None, MF_USERS),
           "rows_P": np.unique(users), "rows_Q": np.unique(np.r_[items, negs] if pairwise else items)}
    for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
        out[tag] = mf_gradients(P, Q, users, items, third, pairwise, kind, dt)
    return _frozen(out)


def mf_cases():
    """every (pairwise, kind, d, batch) the GPU test runs"""
    for pairwise, kind in MF_LOSSES:
        for d in MF_DIMS:
            for B in MF_BATCHES:
                yield pairwise, kind, d, B
        for d in MF_CONSTRUCTED_DIMS:
            for name in MF_CONSTRUCTED:
                yield pairwise, kind, d, name


def hinge_kink():
    """Two triplets on dyadic tables, reg = 1/4: triplet 0 has P[1].(Q[0] - Q[2]) = 5/8 - 13/8 = -1, the hinge argument
    y + 1 is exactly 0 and the derivative there is 0, as learner.py writes it (max(y + 1, 0): the slot contributes its
    regulariser only); triplet 1 has y + 1 = 17/16 > 0.  Q[0] is the positive of both.  Every product and sum is exact
    in float32."""
    P = np.array([[0.5, 0.25, 2.0, 1.0], [1.0, 0.5, 0.0, 0.0], [3.0, 3.0, 3.0, 3.0]], np.float32)
    Q = np.array([[0.5, 0.25, 1.0, 0.5], [2.0, 2.0, 2.0, 2.0], [1.0, 1.25, 0.5, 0.25], [0.25, 0.5, 0.75, 1.0]],
                 np.float32)
    users, pos, neg = (np.array(a, np.int32) for a in ([1, 0], [0, 0], [2, 3]))
    return P, Q, users, pos, neg, 0.25


# ------------------------------------------------------------------ sort keys
SORT_NS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 16383, 16384)


def sort_keys_input(n):
    """n non-negative int64 keys: seven values in the high word (long runs of equal rows), a low word from a small
    range (whole keys repeat too) and the largest key 0x7fffffffffffffff among them"""
    rs = np.random.RandomState(n)
    keys = (rs.randint(0, 7, n).astype(np.int64) << 32) | rs.randint(0, max(n // 2, 2), n).astype(np.int64)
    if n:
        keys[rs.randint(n)] = 0x7fffffffffffffff
    return keys
