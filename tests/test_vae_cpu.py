"""The restatement of the narrow Mult-VAE kernels (tests/vae_restatement.py) checked on the host, so that
test_vae_gpu.py does not compare a kernel with a wrong copy of itself: the float64 stages chained over one batch
reproduce oracle.train.multivae_loss_and_grads (the TF-graph statement of the model) to 1e-10 of scale, the frozen cases
hold the lengths, segment plans and repeats they claim, every float32-to-float64 distance the GPU test uses as a
yardstick is non-zero, the segment order is visible in float32 bits, and the wide logits are legitimate inputs."""
import numpy as np
import pytest

from oracle import train
import vae_restatement as V

ORACLE_TOL = 1e-10            # relative to max|want|: float64 rounds at 1.1e-16, the sums here are a few thousand long
DEC_SHAPES = ((1, 1, 1), (33, 31, 32), (257, 100, 20), (513, 70, 32), (40, 32 * (256 + 3) + 5, 32))


def _close(what, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    rel = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    print("%s: largest difference to the oracle / max|want| = %.3g" % (what, rel))
    assert rel <= ORACLE_TOL, (what, rel)


@pytest.mark.parametrize("act", ["tanh", "sigmoid", "relu"])
def test_chained_float64_stages_reproduce_the_oracle(act):
    """encode -> decoder -> mid_backward -> the small weight gradients -> dwq0 in float64 on the 64-row batch of short
    users (a user appears several times), I cut to the batch's largest item: loss, nll, KL and all eight gradients of
    oracle.train.multivae_loss_and_grads at reg = 0"""
    h, z, keep, anneal = 20, 5, 0.8, 0.2
    indptr, indices = V.bag_csr()
    rows = V.batches()["b64"]
    assert len(set(rows.tolist())) < len(rows)
    I = int(max(indices[indptr[u]:indptr[u + 1]].max() for u in rows if indptr[u + 1] > indptr[u])) + 1
    P = dict(V.params(h, z))
    for k in ("Wq0", "Wp1t", "bp1"):
        P[k] = P[k][:I]
    kept, eps = V.given_draws(z)
    eps = eps[:len(rows)]
    f8 = np.float64
    e = V.encode(indptr, indices, rows, P, V.ACTS[act], keep, kept, eps, 1.0, f8)
    d = V.decoder(indptr, indices, rows, e["G1"], P["Wp1t"], P["bp1"], f8)
    DA3, DH2, DA1 = V.mid_backward(d["dg1"], e["G1"], e["H1"], e["MU"], e["LOGVAR"], e["EPSSTD"], P["Wp0"].astype(f8),
                                   P["Wq1"].astype(f8), V.ACTS[act], anneal)
    dWp0, dbp0, dWq1, dbq1, dbq0 = V.mid_wgrads(e["ZS"], e["H1"], DA3, DH2, DA1)
    dWq0 = V.dwq0(indptr, indices, rows, V.h0_values(indptr, kept, keep, f8), DA1, I)

    X = V.dense_rows(indptr, indices, rows, I, f8)
    D = np.ones_like(X)
    for r, u in enumerate(rows):
        D[r, indices[indptr[u]:indptr[u + 1]]] = kept[indptr[u]:indptr[u + 1]]
    p = {k: v.astype(f8) for k, v in P.items()}
    wl, (gWq, gbq, gWp, gbp), (wnll, wkl) = train.multivae_loss_and_grads(
        X, [p["Wq0"], p["Wq1"]], [p["bq0"], p["bq1"]], [p["Wp0"], p["Wp1t"].T.copy()], [p["bp0"], p["bp1"]], D,
        np.float32(keep), eps.astype(f8), np.float32(anneal), 0.0, act)
    nll, kl = d["nll"].mean(), e["KLb"].mean()
    _close("nll", nll, wnll)
    _close("KL", kl, wkl)
    _close("loss", nll + f8(np.float32(anneal)) * kl, wl)
    for name, got, want in (("Wq0", dWq0, gWq[0]), ("bq0", dbq0, gbq[0]), ("Wq1", dWq1, gWq[1]), ("bq1", dbq1, gbq[1]),
                            ("Wp0", dWp0, gWp[0]), ("bp0", dbp0, gbp[0]), ("Wp1t", d["dWp1"], gWp[1].T),
                            ("bp1", d["dbp1"], gbp[1])):
        _close("d" + name, got, want)


def test_cases_hold_what_they_claim():
    indptr, indices = V.bag_csr()
    n = np.diff(indptr)
    assert tuple(n) == V.BAG_LENGTHS and indices.max() < V.BAG_ITEMS and len(indices) == indptr[-1]
    for u in range(len(n)):
        row = indices[indptr[u]:indptr[u + 1]]
        assert np.all(np.diff(row) > 0)
    for edge in (V.ENC_SEG, V.DWQ0_ROUND, V.ENC_SEG * V.ENC_MAX_SEG):           # 256, 1,024, 16,384
        assert edge in n and edge + 1 in n                  # the last length of one path, the first of the next
    assert V.DWQ0_ROUND == 1024 and 4 * V.ENC_SEG == 1024                       # a wave's second segment, dwq0's 2nd round
    plans = {c: V.seg_plan(c) for c in V.BAG_LENGTHS}
    assert [plans[c][1] for c in (0, 256, 257, 1025, 16384)] == [1, 1, 2, 5, 64]
    assert plans[16384][0] == 256 and plans[16385] == (257, 64) and plans[16500] == (258, 64)
    assert all(ns <= V.ENC_MAX_SEG for _, ns in plans.values())
    b = V.batches()
    assert sorted(b["all"].tolist()) == list(range(len(n)))
    assert not np.array_equal(b["all"], np.sort(b["all"]))
    rep = b["repeat"].tolist()
    assert len(set(rep)) == len(rep) - 1 and V.user_of(1025) in rep and V.user_of(0) in rep
    assert len(b["single"]) == 1
    for size in V.DRAWN_SIZES:
        assert len(b["b%d" % size]) == size and n[b["b%d" % size]].max() <= V.SHORT
    for h, z in V.WIDTHS:
        assert 1 <= h <= 32 and 1 <= 2 * z <= 32
    kept = V.given_draws(16)[0]
    assert 0.75 < kept.mean() < 0.85


def test_device_draws_restate_the_kernel_keys():
    """the keep mask and the noise from Python integers, as vae_encode_kernel writes the keys"""
    seed, step, keep = V.SEED, 5, 0.8
    nnz = 3000
    m = V.keep_mask(seed, step, nnz, keep)
    key = V.splitmix64(seed ^ ((step * 0x9e3779b97f4a7c15) & (2 ** 64 - 1)))
    for t in (0, 1, 17, 1024, 2999):
        u = V.uniform01(np.uint64(V.splitmix64(key ^ t)))
        assert m[t] == np.float32(u < np.float32(keep))
    assert 0.75 < m.mean() < 0.85 and V.keep_mask(seed, step, nnz, 1.0).all()
    assert not np.array_equal(m, V.keep_mask(seed, step + 1, nnz, keep))
    z, r, lane = 5, 7, 3
    e32 = V.noise(seed, step, 12, z, np.float32)
    k0 = V.splitmix64(V.splitmix64(seed ^ 0xabcd ^ (step << 20)) ^ (r * z + lane))
    u1, u2 = V.uniform01(np.uint64(k0)), V.uniform01(np.uint64(V.splitmix64(k0)))
    want = 0.01 * np.sqrt(-2.0 * np.log(float(u1))) * np.cos(float(np.float32(6.2831853)) * float(u2))
    assert abs(e32[r, lane] - want) < 1e-7
    e = V.noise(seed, step, 4000, 16, np.float64)
    assert abs(e.mean()) < 1e-3 and abs(e.std() - 0.01) < 5e-4


def test_float64_small_gradients_are_the_plain_products():
    c = V.mid_inputs(130, 20, 5, "tanh")
    f = lambda k: c[k].astype(np.float64)
    DA3, DH2, DA1 = V.mid_backward(f("dG1"), f("G1"), f("H1"), f("MU"), f("LOGVAR"), f("EPSSTD"), f("Wp0"), f("Wq1"),
                                   0, 0.2)
    dWp0, dbp0, dWq1, dbq1, dbq0 = V.mid_wgrads(f("ZS"), f("H1"), DA3, DH2, DA1)
    for what, got, want in (("dWp0", dWp0, f("ZS").T @ DA3), ("dbp0", dbp0, DA3.sum(0)), ("dWq1", dWq1, f("H1").T @ DH2),
                            ("dbq1", dbq1, DH2.sum(0)), ("dbq0", dbq0, DA1.sum(0))):
        _close(what, got, want)


def _dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def test_every_yardstick_is_non_zero():
    """the float32 restatement's own distance to float64 — what the GPU test multiplies by 4 — on each case whose
    device result is not pinned bit for bit"""
    for h, z in V.WIDTHS:
        for act in ("tanh", "sigmoid"):
            e32 = V.encode_case(h, z, "all", act, 0.8, 1.0, np.float32)
            e64 = V.encode_case(h, z, "all", act, 0.8, 1.0, np.float64)
            for k in ("H1", "MU", "LOGVAR", "EPSSTD", "ZS", "G1", "KLb"):
                assert _dist(e32[k], e64[k]) > 0, (h, z, act, k)
        for act in ("relu", "identity"):
            e32 = V.encode_case(h, z, "all", act, 0.8, 1.0, np.float32)
            e64 = V.encode_case(h, z, "all", act, 0.8, 1.0, np.float64)
            for k in ("EPSSTD", "ZS", "G1", "KLb"):      # (at h = 1 a relu output can be 0 in every row: exact then)
                assert _dist(e32[k], e64[k]) > 0 or (k == "G1" and not np.any(e64[k])), (h, z, act, k)
        for act in V.ACTS:
            for B in V.MID_BATCHES:
                c = V.mid_inputs(B, h, z, act)
                f4 = [c[k] for k in ("dG1", "G1", "H1", "MU", "LOGVAR", "EPSSTD", "Wp0", "Wq1")]
                o32 = V.mid_backward(*f4, V.ACTS[act], 0.2)
                o64 = V.mid_backward(*[x.astype(np.float64) for x in f4], V.ACTS[act], 0.2)
                assert _dist(o32[1], o64[1]) > 0, (h, z, act, B)
                if not (act == "relu" and B == 1):           # one relu row can be all zeros in H1
                    assert _dist(o32[2], o64[2]) > 0 or not np.any(o64[2]), (h, z, act, B)
    for z in (16, 5, 1):                                     # the drawn noise: logf, sqrtf, cosf
        for name in ("all", "repeat"):
            B = len(V.batches()[name])
            for step in (3, 4):
                assert _dist(V.noise(V.SEED, step, B, z, np.float32), V.noise(V.SEED, step, B, z, np.float64)) > 0
    indptr, indices = V.bag_csr()
    for name in ("all", "repeat"):
        rows = V.batches()[name]
        for h in (32, 20, 1):
            rs = np.random.RandomState(h)
            DA1 = rs.randn(len(rows), h).astype(np.float32)
            hv = V.h0_values(indptr, V.given_draws(16)[0], 0.8, np.float32)
            assert _dist(V.dwq0(indptr, indices, rows, hv, DA1, V.BAG_ITEMS),
                         V.dwq0(indptr, indices, rows, hv.astype(np.float64), DA1.astype(np.float64), V.BAG_ITEMS)) > 0
    for B, I, h in DEC_SHAPES[1:]:                           # (1, 1, 1): every output is exactly 0 in both widths
        for kind in V.DEC_KINDS:
            w32, w64 = V.decoder_want(B, I, h, kind, np.float32), V.decoder_want(B, I, h, kind, np.float64)
            for k in ("nll", "dWp1", "dbp1", "dg1"):
                if kind == "flat" and k == "dg1":            # W = 0: dg1 = 0 exactly
                    assert not np.any(w64[k])
                    continue
                assert _dist(w32[k], w64[k]) > 0, (B, I, h, kind, k)
    w64 = V.decoder_want(1, 1, 1, "unit", np.float64)
    assert not np.any(w64["nll"]) and not np.any(w64["G"])


def test_segment_order_is_observable_in_float32():
    """one plain chain over a long row differs in float32 bits from the segmented order the kernel documents"""
    indptr, indices = V.bag_csr()
    P = V.params(32, 16)
    vals = V.h0_values(indptr, V.given_draws(16)[0], 0.8, np.float32)
    for length in (1025, 16500):
        rows = np.array([V.user_of(length)], np.int32)
        seg = V.bag_sums(indptr, indices, rows, P["Wq0"], vals)
        plain = V.bag_sums(indptr, indices, rows, P["Wq0"], vals, segmented=False)
        assert not np.array_equal(seg, plain), length
        assert np.abs(seg - plain).max() < 1e-5
    rows = np.array([V.user_of(256)], np.int32)             # one segment: the same chain
    assert np.array_equal(V.bag_sums(indptr, indices, rows, P["Wq0"], vals),
                          V.bag_sums(indptr, indices, rows, P["Wq0"], vals, segmented=False))


def test_decoder_cases_hold_what_they_claim():
    """wide logits are finite in float64 everywhere and span more than 104 in every row (the clamp of exp_nonpos
    engages); buried positives lie at least 30 under their row's maximum; flat rows have lse = 0.25 + log I; every
    batch from B = 4 on holds the empty user, a user of every item and one user twice"""
    for B, I, h in DEC_SHAPES:
        for kind in V.DEC_KINDS:
            c = V.decoder_case(B, I, h, kind)
            w = V.decoder_want(B, I, h, kind, np.float64)
            assert all(np.all(np.isfinite(w[k])) for k in w), (B, I, h, kind)
            n = np.diff(c["indptr"])[c["rows"]]
            if B >= 4:
                assert 0 in n and len(set(c["rows"].tolist())) == B - 1
                assert (I in n) == (kind != "buried" or I < 31)
            if kind == "wide" and I > 1:
                assert np.all(w["logits"].max(1) - w["logits"].min(1) > 104.0)
            if kind == "flat":
                assert np.abs(w["lse"] - (0.25 + np.log(I))).max() < 1e-12
                assert np.intersect1d(n, V.DEC_POW2).size > 0
            if kind == "buried" and I >= 31:
                X = V.dense_rows(c["indptr"], c["indices"], c["rows"], I, np.float64)
                top = w["logits"].max(1, keepdims=True)
                assert np.all((top - w["logits"])[X > 0] >= 30.0) and X.sum() > 0
