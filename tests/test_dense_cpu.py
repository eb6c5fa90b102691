"""The restatement of the width-generic dense kernels (tests/dense_restatement.py) checked on the host, so that
test_dense_gpu.py does not compare a kernel with a wrong copy of itself: the float64 backward functions against
torch.autograd in float64 on forwards written independently with torch ops (bound: AUTOGRAD_TOL relative to the
largest gradient — float64 rounds at 1.1e-16; the largest value seen is 4.4e-15, the softmax gradient behind a
log-sum-exp near 80, and each is printed), the float32 forms within ordinary
rounding of their float64 forms, the single-rounding fmaf, the hash and the split-K restatement against
oracle.native.score_gemm, and the constructed inputs shown to hold what they claim."""
import numpy as np
import pytest
import torch

from oracle import native
import dense_restatement as R

AUTOGRAD_TOL = 1e-13          # relative to max|gradient|: float64 keeps 2^-53 = 1.1e-16 per operation
SEEN = {}


def _close64(what, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rel = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    SEEN[what] = rel
    print("%s: largest difference to autograd / max|gradient| = %.3g (bound %.0e)" % (what, rel, AUTOGRAD_TOL))
    assert got.shape == want.shape and rel <= AUTOGRAD_TOL, (what, rel)


def _t(a, grad=True):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def _lrelu(x):
    return torch.where(x > 0, x, x * float(R.LEAKY))


# ------------------------------------------------------------------ building blocks
def test_fmaf_is_one_rounding():
    """against the C fmaf of oracle.native.score_gemm (a chain of two steps: acc = fmaf(a1, b1, fmaf(a0, b0, 0))) on
    random operands and on one case built so that the float64 sum a b + c lands exactly between two float32 although
    the exact sum does not: c = 1 + 2^-23, a b = 2^-24 - 2^-70.  Rounding the float64 sum again gives 1 + 2^-22 (the
    even neighbour), one rounding gives 1 + 2^-23."""
    rs = np.random.RandomState(0)
    n = 2000
    a0, b0, a1, b1 = (rs.randn(n).astype(np.float32) for _ in range(4))
    a0[0], b0[0] = 1.0 + 2.0 ** -23, 1.0
    a1[0], b1[0] = 2.0 ** -24 * (1.0 + 2.0 ** -23), 1.0 - 2.0 ** -23
    want = native.score_gemm(np.stack([a0, a1], 1), None, np.stack([b0, b1], 1)).diagonal()
    first = R.fmaf(a0, b0, np.zeros(n, np.float32))
    assert np.array_equal(first, a0 * b0)
    got = R.fmaf(a1, b1, first)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    twice = (a1.astype(np.float64) * b1.astype(np.float64) + first.astype(np.float64)).astype(np.float32)
    assert got[0] == np.float32(1.0 + 2.0 ** -23) and twice[0] == np.float32(1.0 + 2.0 ** -22)
    x64 = rs.randn(5)
    assert np.array_equal(R.fmaf(x64, x64, x64), x64 * x64 + x64)
    assert R.fmaf(np.float32(2), np.float32(3), np.float32(1)).shape == ()


def test_fma_chain_and_the_unsplit_product_equal_score_gemm():
    rs = np.random.RandomState(1)
    A, B = rs.randn(9, 37).astype(np.float32), rs.randn(13, 37).astype(np.float32)
    want = native.score_gemm(A, None, B)
    assert np.array_equal(R.fma_chain(A, B), want)
    assert np.array_equal(R.gemm(A, B, splits=1), want)
    C0 = rs.randn(9, 13).astype(np.float32)
    cont = R.gemm(A, B, splits=1, C0=C0)
    assert not np.array_equal(cont, C0 + want)                       # continued from C, not added afterwards
    assert np.abs(cont.astype(np.float64) - (C0 + A.astype(np.float64) @ B.astype(np.float64).T)).max() < 1e-5
    assert np.abs(R.gemm(A.astype(np.float64), B.astype(np.float64), 1, C0.astype(np.float64)) - cont).max() < 1e-5


def test_split_plan_and_association():
    """the issue's (K, splits): 65 parts of 16; used = 63 <= 64 < splits; 97 parts of 208; the production 277 parts of
    256.  Two-level sums differ in bits from one left-to-right pass, and accumulate adds C first."""
    assert R.split_plan(1040, 65) == (16, 65) and R.split_plan(1000, 100) == (16, 63)
    assert R.split_plan(20000, 100) == (208, 97) and R.split_plan(70839, 277) == (256, 277)
    assert R.split_plan(1024, 64) == (16, 64) and R.split_plan(5000, 8) == (640, 8)
    rs = np.random.RandomState(2)
    A, B = rs.randn(24, 20000).astype(np.float32), rs.randn(40, 20000).astype(np.float32)
    C0 = rs.randn(24, 40).astype(np.float32)
    per, used = R.split_plan(20000, 100)
    parts = [native.score_gemm(A[:, s * per:(s + 1) * per], None, B[:, s * per:(s + 1) * per]) for s in range(used)]
    flat = np.zeros((24, 40), np.float32)
    for p in parts:
        flat = flat + p
    two = R.gemm(A, B, splits=100)
    assert not np.array_equal(two, flat)
    want64 = A.astype(np.float64) @ B.astype(np.float64).T
    assert np.abs(two - want64).max() <= 2e-6 * np.sqrt(20000) * np.abs(want64).max()
    per64, used64 = R.split_plan(20000, 64)                            # at most 64 splits: one level, left to right
    one = np.zeros((24, 40), np.float32)
    for s in range(used64):
        one = one + native.score_gemm(A[:, s * per64:(s + 1) * per64], None, B[:, s * per64:(s + 1) * per64])
    assert used64 == 63 and np.array_equal(R.gemm(A, B, splits=64), one)
    after = two + C0
    first = R.gemm(A, B, splits=100, C0=C0)
    assert not np.array_equal(first, after) and np.abs(first - after).max() < 1e-3
    b = rs.randn(40).astype(np.float32)
    assert np.array_equal(R.gemm(A, B, splits=100, bias=b, act=2), np.maximum(two + b[None, :], 0))
    assert np.abs(R.gemm(A.astype(np.float64), B.astype(np.float64), 100) - want64).max() <= 1e-9


def test_hash_on_arrays_equals_python_integers():
    rs = np.random.RandomState(3)
    xs = [0, 1, R.M64, 0x8000000000000000] + [int(x) for x in rs.randint(0, 2 ** 62, 50)] + [2 ** 63 + 12345]
    got = R.splitmix64_array(np.array(xs, np.uint64))
    assert [int(g) for g in got] == [R.splitmix64(x) for x in xs]
    assert R.splitmix64(0) == 0xe220a8397b1dcdaf                        # the published first output of SplitMix64
    key = R.layer_mask_key(2017, 5, 2)
    m = R.draw_mask(key, 300, 0.9)
    want = [int(np.float32(R.splitmix64(key ^ e) >> 40) * np.float32(2.0 ** -24) < np.float32(0.9)) for e in range(300)]
    assert m.tolist() == want and 0 < m.sum() < 300
    for other in (R.layer_mask_key(2017, 6, 2), R.layer_mask_key(2017, 5, 3), R.edge_mask_key(2017, 5),
                  R.bag_drop_key(2017, 5)):
        assert other != key and not np.array_equal(R.draw_mask(other, 300, 0.9), m)
    assert R.draw_mask(key, 300, 1.0).all()
    # uniform01 rounds its + 0.5 in float32: the largest 24-bit value gives exactly 1.0, which is not below keep = 1
    assert R.uniform01(np.array([R.M64], np.uint64))[0] == 1.0 and R.uniform01(np.array([0], np.uint64))[0] == 2.0 ** -25
    assert R.draw_bag_keep(key, 50, 1.0).all() and 0 < R.draw_bag_keep(key, 500, 0.8).sum() < 500


def test_tree_sum_is_the_xor_butterfly():
    rs = np.random.RandomState(4)
    v = rs.randn(7, 64).astype(np.float32)
    x = v.copy()
    for m in (32, 16, 8, 4, 2, 1):
        x = x + x[:, np.arange(64) ^ m]
    assert np.all(x == x[:, :1]) and np.array_equal(R.tree_sum(v), x[:, 0])
    s = rs.randn(1024).astype(np.float32)
    red = s.copy()
    k = 512
    while k >= 1:
        red[:k] += red[k:2 * k]
        k //= 2
    assert R.tree_sum(s) == red[0]


# ------------------------------------------------------------------ backward restatements against autograd
@pytest.mark.parametrize("w", [1, 24, 65, 200])
def test_ngcf_act_bwd_equals_autograd(w):
    """l2_normalize(dropout(lrelu(T1) + lrelu(T2))) with the loss sum(out * d_out) + sum(E' * d_ego_next), a row whose
    squared norm is below 1e-12 (there max(ss, 1e-12) is flat and the gradient is g / sqrt(1e-12)) and a zero row"""
    c = R.ngcf_inputs(5, w)
    f = lambda k: c[k].astype(np.float64)
    keep = float(np.float32(0.9))
    T1, T2 = _t(f("T1")), _t(f("T2"))
    m = _t(c["mask"], False)
    ego = (_lrelu(T1) + _lrelu(T2)) / keep * m
    ss = (ego * ego).sum(1, keepdim=True)
    out = ego / torch.sqrt(torch.clamp(ss, min=float(R.NORM_EPS)))
    sd = ss.detach().numpy()[:, 0]
    assert 0 < sd[R.ROW_TINY] < 1e-12 and sd[R.ROW_ZERO] == 0 and sd[3:].min() > 1e-3
    for given in (True, False):
        loss = (out * _t(f("d_out"), False)).sum()
        if given:
            loss = loss + (ego * _t(f("d_ego_next"), False)).sum()
        g1, g2 = torch.autograd.grad(loss, (T1, T2), retain_graph=True)
        e64, o64 = R.ngcf_act_fwd(f("T1"), f("T2"), c["mask"], 0.9)
        assert np.abs(e64 - ego.detach().numpy()).max() <= 1e-15 and np.abs(o64 - out.detach().numpy()).max() <= 1e-9
        d1, d2 = R.ngcf_act_bwd(f("d_out"), f("d_ego_next") if given else None, e64, f("T1"), f("T2"), c["mask"], 0.9)
        # torch's leaky slope at exactly 0 is taken from the x * 0.2 branch, as the kernel's (t > 0 ? dz : dz * 0.2)
        _close64("ngcf_act_bwd dT1 w=%d next=%s" % (w, given), d1, g1.numpy())
        _close64("ngcf_act_bwd dT2 w=%d next=%s" % (w, given), d2, g2.numpy())


def test_ngcf_mix_bwd_equals_autograd():
    """T1 = S W_gc, T2 = (ego .* S) W_bi: with Y1 = dT1 W_gc^T and Y2 = dT2 W_bi^T the gradient to S is Y1 + Y2 .* ego
    and the direct gradient to ego is Y2 .* S"""
    c = R.ngcf_inputs(5, 24)
    f = lambda k: c[k].astype(np.float64)
    S, ego = _t(f("S")), _t(f("ego"))
    loss = (S * _t(f("Y1"), False)).sum() + (ego * S * _t(f("Y2"), False)).sum()
    gS, gE = torch.autograd.grad(loss, (S, ego))
    dS, dE = R.ngcf_mix_bwd(f("Y1"), f("Y2"), f("ego"), f("S"), 32)
    _close64("ngcf_mix_bwd dS", dS[:, :24], gS.numpy())
    _close64("ngcf_mix_bwd d_ego", dE[:, :24], gE.numpy())
    assert not dS[:, 24:].any() and not dE[:, 24:].any() and dS.shape == (5, 32)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_lrelu_drop_bwd_equals_autograd(flags):
    c = R.ngcf_inputs(5, 65)
    f = lambda k: c[k].astype(np.float64)
    keep = float(np.float32(0.9))
    T = _t(f("T1"))
    y = _lrelu(T) if flags & 1 else T
    if flags & 2:
        y = y / keep * _t(c["mask"], False)
    assert np.abs(R.lrelu_drop_fwd(f("T1"), c["mask"], 0.9, flags) - y.detach().numpy()).max() <= 1e-15
    for with_b in (False, True):
        loss = (y * _t(f("d_a"), False)).sum() + ((y * _t(f("d_b"), False)).sum() if with_b else 0)
        g, = torch.autograd.grad(loss, (T,), retain_graph=True)
        got = R.lrelu_drop_bwd(f("d_a"), f("d_b") if with_b else None, f("T1"), c["mask"], 0.9, flags)
        _close64("lrelu_drop_bwd flags=%d b=%s" % (flags, with_b), got, g.numpy())


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_act_bwd_equals_autograd(act):
    rs = np.random.RandomState(act)
    x, dY = rs.randn(300), rs.randn(300)
    X = _t(x)
    Y = {0: torch.tanh, 1: torch.sigmoid, 2: torch.relu, 3: lambda v: v * 1.0}[act](X)
    g, = torch.autograd.grad((Y * _t(dY, False)).sum(), (X,))
    y64 = R.act_fwd(act, x)
    assert np.abs(y64 - Y.detach().numpy()).max() <= 1e-15
    _close64("act_bwd act=%d" % act, R.act_bwd(act, dY, y64), g.numpy())


@pytest.mark.parametrize("anneal", [0.0, 0.2])
def test_vae_sample_bwd_equals_autograd(anneal):
    """loss = sum(ZS * dZ) + anneal * mean_b KL_b with ZS = mu + eps * exp(logvar / 2) (training) and
    KL_b = 1/2 sum(-logvar + exp(logvar) + mu^2 - 1)"""
    rs = np.random.RandomState(5)
    B, z = 5, 65
    H2, eps, dZ = 0.5 * rs.randn(B, 2 * z), 0.01 * rs.randn(B, z), rs.randn(B, z)
    a = float(np.float32(anneal))
    H = _t(H2)
    mu, logvar = H[:, :z], H[:, z:]
    ZS = mu + _t(eps, False) * torch.exp(0.5 * logvar)
    KL = 0.5 * (-logvar + torch.exp(logvar) + mu * mu - 1).sum(1)
    g, = torch.autograd.grad((ZS * _t(dZ, False)).sum() + a * KL.mean(), (H,))
    es, zs, kl = R.vae_sample(H2, eps, 1.0)
    assert np.abs(zs - ZS.detach().numpy()).max() <= 1e-15 and np.abs(kl - KL.detach().numpy()).max() <= 1e-13
    assert np.array_equal(R.vae_sample(H2, eps, 0.0)[1], H2[:, :z])
    _close64("vae_sample_bwd anneal=%g" % anneal, R.vae_sample_bwd(dZ, H2, es, anneal), g.numpy())


def test_softmax_dlogits_equals_autograd():
    """loss = mean over the batch of -sum over the row's items of log_softmax(logits); rows with 0, 1, 1023, 1024 and
    1025 items, a logit near 80 in each, and a row of ordinary logits with 37 items"""
    S, items, ld = R.softmax_case(2500)
    X = _t(S[:, :2500])
    ls = torch.log_softmax(X, dim=1)
    nll = torch.stack([-(ls[r, torch.tensor(items[r], dtype=torch.long)]).sum() for r in range(len(items))])
    g, = torch.autograd.grad(nll.mean(), (X,))
    n64, d64 = R.softmax_dlogits(S[:, :2500].astype(np.float64), items)
    _close64("softmax nll", n64, nll.detach().numpy())
    _close64("softmax dlogits", d64, g.numpy())
    assert not d64[0].any() and [len(i) for i in items] == list(R.SOFTMAX_ITEM_COUNTS) and ld == 2560
    # the ordinary row: its gradient is spread over the columns, the others' sit on their largest logit
    plain = np.abs(d64[R.SOFTMAX_PLAIN_ROW])
    assert (plain > 1e-3 * plain.max()).sum() > 1000 and (np.abs(d64[1]) > 1e-3 * np.abs(d64[1]).max()).sum() <= 2


# ------------------------------------------------------------------ float32 within float64
def _rounding(what, w32, w64, ops):
    """|float32 form - float64 form| <= ops * 2^-24 * max|float64 form|, and not zero (the GPU bound is a multiple)"""
    err = np.abs(np.asarray(w32, np.float64) - w64).max()
    assert w32.dtype == np.float32 and w64.dtype == np.float64
    assert 0 < err <= ops * 2.0 ** -24 * np.abs(w64).max(), (what, err, np.abs(w64).max())


def test_float32_restatements_lie_within_rounding_of_float64():
    """ops: a generous count of roundings each output passes through (sums count their terms once)"""
    c = R.ngcf_inputs(1001, 200)
    f = lambda k: c[k].astype(np.float64)
    e32, o32 = R.ngcf_act_fwd(c["T1"], c["T2"], c["mask"], 0.9, 256)
    e64, o64 = R.ngcf_act_fwd(f("T1"), f("T2"), c["mask"], 0.9, 256)
    _rounding("act_fwd ego", e32, e64, 4)
    _rounding("act_fwd out", o32, o64, 16)
    b32 = R.ngcf_act_bwd(c["d_out"], c["d_ego_next"], e32[:, :200], c["T1"], c["T2"], c["mask"], 0.9)
    b64 = R.ngcf_act_bwd(f("d_out"), f("d_ego_next"), e32[:, :200].astype(np.float64), f("T1"), f("T2"), c["mask"], 0.9)
    # the tiny row's gradient is 1e6 g: relative to the largest, as everywhere
    _rounding("act_bwd dT1", b32[0], b64[0], 64)
    _rounding("act_bwd dT2", b32[1], b64[1], 64)
    _rounding("mix_bwd", R.ngcf_mix_bwd(c["Y1"], c["Y2"], c["ego"], c["S"], 256)[0],
              R.ngcf_mix_bwd(f("Y1"), f("Y2"), f("ego"), f("S"), 256)[0], 4)
    _rounding("lrelu_drop_fwd", R.lrelu_drop_fwd(c["T1"], c["mask"], 0.9, 3), R.lrelu_drop_fwd(f("T1"), c["mask"], 0.9, 3), 4)
    _rounding("lrelu_drop_bwd", R.lrelu_drop_bwd(c["d_a"], c["d_b"], c["T1"], c["mask"], 0.9, 3),
              R.lrelu_drop_bwd(f("d_a"), f("d_b"), f("T1"), c["mask"], 0.9, 3), 8)
    _rounding("edge_dropout", R.edge_dropout(c["S"], c["mask"], 0.9), R.edge_dropout(f("S"), c["mask"], 0.9), 4)
    rs = np.random.RandomState(6)
    X = rs.randn(2561, 65).astype(np.float32)
    _rounding("colsum_rows", R.colsum_rows(X), R.colsum_rows(X.astype(np.float64)), 2561)
    assert np.abs(R.colsum_rows(X.astype(np.float64)) - X.astype(np.float64).sum(0)).max() <= 1e-11
    H2, eps = (0.5 * rs.randn(130, 400)).astype(np.float32), (0.01 * rs.randn(130, 200)).astype(np.float32)
    for k, (a, b) in enumerate(zip(R.vae_sample(H2, eps, 1.0), R.vae_sample(H2.astype(np.float64), eps.astype(np.float64), 1.0))):
        _rounding("vae_sample %d" % k, a, b, (16, 16, 400)[k])
    dZ = rs.randn(130, 200).astype(np.float32)
    es = R.vae_sample(H2, eps, 1.0)[0]
    _rounding("vae_sample_bwd", R.vae_sample_bwd(dZ, H2, es, 0.2),
              R.vae_sample_bwd(dZ.astype(np.float64), H2.astype(np.float64), es.astype(np.float64), 0.2), 16)
    S, items, _ = R.softmax_case(1025)
    for k, (a, b) in enumerate(zip(R.softmax_dlogits(S[:, :1025], items), R.softmax_dlogits(S[:, :1025].astype(np.float64), items))):
        _rounding("softmax %d" % k, a, b, 4096)
    for act in range(4):
        y = R.act_fwd(act, X)
        _rounding("act_bwd %d" % act, R.act_bwd(act, X[::-1].copy(), y) if act < 2 else R.act_bwd(act, X[::-1] * np.float32(1.1), y),
                  R.act_bwd(act, X[::-1].astype(np.float64) * (1.0 if act < 2 else float(np.float32(1.1))), y.astype(np.float64)), 8)
    indptr, indices, rows = R.bag_csr()
    W, bias = rs.randn(R.BAG_ITEMS, 65).astype(np.float32), rs.randn(65).astype(np.float32)
    kept = R.draw_bag_keep(R.bag_drop_key(7, 3), len(indices), 0.8)
    r32 = R.vae_bag_fwd(indptr, indices, rows, W, bias, 0, 0.8, kept)
    r64 = R.vae_bag_fwd(indptr, indices, rows, W.astype(np.float64), bias.astype(np.float64), 0, 0.8, kept)
    _rounding("bag h0val", r32[1], r64[1], 4)
    _rounding("bag pre", r32[2], r64[2], 129)
    _rounding("bag tanh", r32[3], r64[3], 129)
    for dt in (np.float32, np.float64):
        e = R.draw_eps(2017, 3, 130, 65, dt)
        assert e.dtype == dt and 0.008 < e.std() < 0.012 and abs(e.mean()) < 1e-3
    _rounding("eps draw", R.draw_eps(2017, 3, 130, 65, np.float32), R.draw_eps(2017, 3, 130, 65, np.float64), 64)


def test_bag_fwd_and_dwq0_equal_the_dense_multi_hot_products():
    """float64, with nothing of the restatement's loops: the batch users' multi-hot rows X [B][I] densified,
    l2_normalize (x / sqrt(max(sum x^2, 1e-12))), dropout x / keep * mask per entry, act(X W + b) as one matrix product
    is vae_bag_fwd, its entries at the batch's CSR positions are h0val, and dW + X^T dA1 is dwq0_wide (one user is
    named twice and counts twice).  h0val is NaN outside the batch's positions: dwq0_wide reads none of them."""
    indptr, indices, rows = R.bag_csr()
    rs = np.random.RandomState(12)
    W, bias = rs.randn(R.BAG_ITEMS, 65), rs.randn(65)
    keep = float(np.float32(0.8))
    kept = R.draw_bag_keep(R.bag_drop_key(7, 3), len(indices), 0.8)
    X, Mk = np.zeros((len(rows), R.BAG_ITEMS)), np.zeros((len(rows), R.BAG_ITEMS))
    spans = [(int(indptr[u]), int(indptr[u + 1])) for u in rows]
    for r, (b, e) in enumerate(spans):
        X[r, indices[b:e]] = 1
        Mk[r, indices[b:e]] = kept[b:e]
    Xd = X / np.sqrt(np.maximum((X * X).sum(1, keepdims=True), float(R.NORM_EPS))) / keep * Mk
    want_pre = Xd @ W + bias
    pos, vals, pre, Y = R.vae_bag_fwd(indptr, indices, rows, W, bias, 0, 0.8, kept)
    assert np.array_equal(pos, np.concatenate([np.arange(b, e) for b, e in spans]))
    assert np.abs(vals - np.concatenate([Xd[r, indices[b:e]] for r, (b, e) in enumerate(spans)])).max() <= 1e-15
    assert np.abs(pre - want_pre).max() <= 1e-13 * np.abs(want_pre).max()
    assert np.abs(Y - np.tanh(want_pre)).max() <= 1e-13
    assert np.array_equal(pre[-1], pre[list(rows).index(rows[-1])]) and list(rows).index(rows[-1]) < len(rows) - 1
    h0 = np.full(len(indices), np.nan)
    h0[pos] = vals
    DA1, dW = rs.randn(len(rows), 65), rs.randn(R.BAG_ITEMS, 65)
    got = R.dwq0_wide(indptr, indices, rows, h0, DA1, dW.copy())
    want = dW + Xd.T @ DA1
    assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


# ------------------------------------------------------------------ the constructed inputs
def test_inputs_hold_what_they_claim():
    indptr, indices, rows = R.bag_csr()
    counts = np.diff(indptr)
    assert sorted(counts[rows].tolist()) == sorted(list(R.BAG_ITEM_COUNTS) + [9])
    assert len(np.unique(rows)) == len(rows) - 1 and np.all(np.abs(np.diff(np.sort(np.unique(rows)))) >= 2)
    for u in range(len(counts)):
        it = indices[indptr[u]:indptr[u + 1]]
        assert np.all(np.diff(it) > 0) and (len(it) == 0 or it.max() < R.BAG_ITEMS)
    named = np.zeros(len(indices), bool)
    for u in rows:
        named[indptr[u]:indptr[u + 1]] = True
    assert 0 < named.sum() < len(named)                              # CSR positions outside the batch exist
    for w in R.NGCF_WIDTHS:
        c = R.ngcf_inputs(5, w)
        e, _ = R.ngcf_act_fwd(c["T1"], c["T2"], c["mask"], 0.9)
        ss = (e.astype(np.float64) ** 2).sum(1)
        assert ss[R.ROW_ZERO] == 0 and ss[R.ROW_MASKED] == 0 and not c["mask"][R.ROW_MASKED].any()
        assert 0 < ss[R.ROW_TINY] < 0.1 * float(R.NORM_EPS) and np.all((ss[3:] == 0) | (ss[3:] > 1e-3))
        assert (c["T1"] == 0).any() and (c["T1"] < 0).any() or w == 1
    for cols in (1, 700, 1024, 1025, 2500):
        S, items, ld = R.softmax_case(cols)
        assert ld % 64 == 0 and ld > cols and np.all(S[:, cols:] == 7.0) and S[:, :cols].max() >= 80
        assert [len(i) for i in items] == [min(c, cols) for c in R.SOFTMAX_ITEM_COUNTS]
        assert np.abs(S[R.SOFTMAX_PLAIN_ROW, :cols]).max() <= 3 and S[:5, :cols].max(1).min() >= 80
