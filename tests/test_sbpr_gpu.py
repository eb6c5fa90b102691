"""SBPR on the GPU (csrc/sbpr.hip through neurec_amd/sbpr.py): the social sets against the reference's and the
restatement's, in one block and in several; the rules, the determinism and the uniformity of an epoch's instances and
the fallback draw; every step of the reference class's trace and predict(); the widths, the batch sizes and the
coinciding items against the float64 restatement; the drop-in run through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from neurec_amd import defaults
import sbpr_restatement as P
from sbpr_restatement import CASES
from test_sbpr_cpu import FIELDS, second_graph

pytestmark = pytest.mark.gpu

LR = 0.05            # gd steps of the edge tests: a gradient term of size 0.1 moves a table by 5e-3, far above the bound


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_sbpr")


def _engine(g, case="bpr_adam", **kw):
    from neurec_amd.sbpr import SBPREngine
    loss, learner = CASES[case]
    return SBPREngine(g["P_0"], g["Q_0"], g["b_0"], (g["indptr"], g["indices"]), (g["trust_indptr"], g["trust_indices"]),
                      float(g["learning_rate"]), float(g["reg_mf"]), 64, loss=loss, learner=learner, **kw)


@pytest.fixture(scope="module")
def stream_engine(golden):
    return _engine(golden, seed=11)


def _small_engine(tr, trust, n_users, n_items, d=4, **kw):
    from neurec_amd.sbpr import SBPREngine
    z = lambda *s: np.zeros(s, np.float32)
    return SBPREngine(z(n_users, d), z(n_items, d), z(n_items), tr, trust, 0.01, 0.0, 8, **kw)


def _host_sets(eng):
    return tuple(t.cpu().numpy() for t in eng.social_sets())


def _batch(g, case, k):
    return tuple(g["%s_%s" % (case, f)][k] for f in FIELDS)


def _dev(eng, users, items, social, neg, suk):
    import torch
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(eng.P.device, dt)
    return tuple(t(a, torch.int32) for a in (users, items, social, neg)) + (t(suk, torch.float32),)


def _feed(eng, batch, loss2):
    eng.step(*_dev(eng, *batch), loss2)
    return float(loss2.cpu().numpy().astype(np.float64).sum())


def _tables(eng):
    return [getattr(eng, k).cpu().numpy() for k in P.TABLES]


# ------------------------------------------------------------------ the sets
def test_sets_equal_the_reference_sets(golden):
    g = golden
    eng = _engine(g)
    ptr, items, counts = _host_sets(eng)
    assert np.array_equal(ptr, g["social_ptr"]) and np.array_equal(items, g["social_items"])
    want = P.sets_as_csr(P.social_sets(g["indptr"], g["indices"], g["trust_indptr"], g["trust_indices"]), 157)
    assert np.array_equal(counts, want[2]) and counts.dtype == np.int32 and eng.n_blocks == 1
    assert np.array_equal(eng.eligible_users.cpu().numpy(), np.flatnonzero(np.diff(g["social_ptr"]) > 0))


def _expansion_sizes(R, s_ptr, s_idx):
    deg = np.diff(R.indptr)
    return np.asarray([deg[s_idx[s_ptr[u]:s_ptr[u + 1]]].sum() if deg[u] else 0 for u in range(R.shape[0])])


def test_sets_on_the_second_graph_in_one_block_and_in_many(golden):
    """a graph with edges to users without train items: equal to the restatement's with the default workspace, and
    with the workspace forced down to the largest single expansion — at least three blocks — and with half of the
    users' segments above the one-launch sort's limit as well; then one pair less of workspace is refused by the
    user's name"""
    from neurec_amd.sbpr import SBPREngine
    R, _, (s_ptr, s_idx) = second_graph(golden)
    U, I = R.shape
    want = P.sets_as_csr(P.social_sets(R.indptr, R.indices, s_ptr, s_idx), U)
    sizes = _expansion_sizes(R, s_ptr, s_idx)
    z = lambda *s: np.zeros(s, np.float32)
    make = lambda **kw: SBPREngine(z(U, 4), z(I, 4), z(I), R, (s_ptr, s_idx), 0.01, 0.0, 8, **kw)
    one = make()
    many = make(workspace_pairs=int(sizes.max()))
    assert one.n_blocks == 1 and many.n_blocks >= 3, many.blocks
    assert all(n <= sizes.max() for _, _, n in many.blocks) and sum(n for _, _, n in many.blocks) == sizes.sum()
    # users above segment_pairs keys are sorted one by one, the others in one segmented launch
    split = make(workspace_pairs=int(sizes.max()), segment_pairs=int(np.median(sizes[sizes > 0])))
    for eng in (one, many, split):
        for got, w in zip(_host_sets(eng), want):
            assert np.array_equal(got, w)
    with pytest.raises(ValueError, match="user %d hold %d items, more than the workspace of %d pairs"
                       % (int(sizes.argmax()), sizes.max(), sizes.max() - 1)):
        make(workspace_pairs=int(sizes.max()) - 1)


def test_a_user_alone_in_a_block():
    """three users in a ring of trust, two items each, a workspace of two pairs: every block holds one user"""
    tr = (np.asarray([0, 2, 4, 6], np.int64), np.asarray([0, 1, 1, 2, 3, 4], np.int32))
    trust = (np.asarray([0, 1, 2, 3], np.int64), np.asarray([1, 2, 0], np.int32))
    eng = _small_engine(tr, trust, 3, 6, workspace_pairs=2)
    assert eng.blocks == [(0, 1, 2), (1, 2, 2), (2, 3, 2)]
    ptr, items, counts = _host_sets(eng)
    assert ptr.tolist() == [0, 1, 3, 5] and items.tolist() == [2, 3, 4, 0, 1] and counts.tolist() == [1] * 5


def test_a_user_with_no_free_item_is_refused_when_the_sets_are_built():
    tr = (np.asarray([0, 2, 4, 5], np.int64), np.asarray([0, 1, 2, 3, 0], np.int32))
    trust = (np.asarray([0, 1, 1, 2], np.int64), np.asarray([1, 1], np.int32))
    with pytest.raises(ValueError, match="user 0 has no item outside"):
        _small_engine(tr, trust, 3, 4)


# ------------------------------------------------------------------ the stream
def _epoch(eng, epoch):
    return tuple(t.cpu().numpy() for t in eng.sample_epoch(epoch))


def test_an_epoch_obeys_the_instance_rules(golden, stream_engine):
    g, eng = golden, stream_engine
    sets = P.social_sets(g["indptr"], g["indices"], g["trust_indptr"], g["trust_indices"])
    users, items, social, neg, suk = _epoch(eng, 0)
    assert len(users) == eng.n_instances == len(g["epoch_users"]) and suk.dtype == np.float32
    for u, i, k, j, s in zip(users, items, social, neg, suk):
        own = g["indices"][g["indptr"][u]:g["indptr"][u + 1]]
        c_items, c_counts = sets[int(u)]                           # KeyError: the user is not eligible
        assert i in own and k in c_items and s == c_counts[np.searchsorted(c_items, k)] + 1
        assert 0 <= j < 131 and j not in own and j not in c_items
    want = P.eligible_positives(g["indptr"], g["indices"], sets)
    assert sorted(zip(users.tolist(), items.tolist())) == sorted(want)
    assert list(zip(users.tolist(), items.tolist())) != want        # permuted
    plain = tuple(t.cpu().numpy() for t in eng.sample_epoch(0, shuffle=False))
    assert list(zip(plain[0].tolist(), plain[1].tolist())) == want  # train_dict order underneath


def test_epochs_differ_and_repeat(golden, stream_engine):
    a, b, c = _epoch(stream_engine, 3), _epoch(stream_engine, 4), _epoch(_engine(golden, seed=11), 3)
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(np.sort(a[3]), np.sort(b[3]))
    for x, y in zip(a, c):
        assert np.array_equal(x, y)
    other = _epoch(_engine(golden, seed=12), 3)
    assert not np.array_equal(a[0], other[0])


def test_a_user_with_one_free_item_always_gets_it():
    """2,000 items: user 0 holds 0..999, the user they trust holds every other item but 1234 — the rejection loop
    finds 1234 in 64 attempts three times in a hundred, so nearly every slot takes the counting fallback"""
    I = 2000
    theirs = np.asarray([i for i in range(1000, I) if i != 1234], np.int32)
    tr = (np.asarray([0, 1000, 1000 + len(theirs)], np.int64), np.concatenate([np.arange(1000, dtype=np.int32), theirs]))
    trust = (np.asarray([0, 1, 1], np.int64), np.asarray([1], np.int32))
    eng = _small_engine(tr, trust, 2, I)
    assert eng.eligible_users.tolist() == [0] and eng.n_instances == 1000
    for epoch in (0, 1):
        users, items, social, neg, suk = _epoch(eng, epoch)
        assert np.all(neg == 1234) and np.all(users == 0) and np.all(suk == 2.0)
        assert sorted(items.tolist()) == list(range(1000)) and np.isin(social, theirs).all()


def test_draws_are_uniform(golden, stream_engine):
    """the user with the largest social set, over enough epochs that every cell of k and of j expects at least 50
    draws: every cell within 5 binomial standard deviations (the draws are a function of the seed: deterministic)"""
    import torch
    g, eng = golden, stream_engine
    sets = P.social_sets(g["indptr"], g["indices"], g["trust_indptr"], g["trust_indices"])
    u = max(sorted(sets), key=lambda x: len(sets[x][0]))
    own = g["indices"][g["indptr"][u]:g["indptr"][u + 1]]
    free = np.setdiff1d(np.arange(131), np.concatenate([own, sets[u][0]]))
    epochs = int(np.ceil(50.0 * max(len(sets[u][0]), len(free)) / len(own)))
    ks, js = [], []
    for e in range(epochs):
        users, _, social, neg, _ = eng.sample_epoch(100 + e)
        pick = users == int(u)
        ks.append(social[pick])
        js.append(neg[pick])
    n = epochs * len(own)
    for draws, cells in ((torch.cat(ks).cpu().numpy(), sets[u][0]), (torch.cat(js).cpu().numpy(), free)):
        assert len(draws) == n
        counts = np.asarray([(draws == c).sum() for c in cells])
        p = 1.0 / len(cells)
        assert counts.sum() == n and n * p >= 50
        worst = np.abs(counts - n * p).max() / np.sqrt(n * p * (1 - p))
        print("user %d: %d cells, %d draws, worst cell %.2f sigma" % (u, len(cells), n, worst))
        assert worst <= 5.0


# ------------------------------------------------------------------ the step
@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Tables and loss after every step against the f64 trace: within 4x the reference's own f32-to-f64 distance of
    that step and table (read from the golden) plus 1e-5 max|want|.  Rows outside <case>_rows_* are bit-equal to their
    initial value; the gradient buffers are zero again afterwards."""
    import torch
    g = golden
    eng = _engine(g, case)
    loss2 = torch.zeros(2, device=eng.P.device)
    for k in range(len(g[case + "_users"])):
        loss = _feed(eng, _batch(g, case, k), loss2)
        want, ref32 = g[case + "_f64_loss"][k], g[case + "_f32_loss"][k]
        print("%s step %d loss: device err %.3g, reference f32 err %.3g" % (case, k + 1, abs(loss - want),
                                                                           abs(ref32 - want)))
        assert abs(loss - want) <= 4 * abs(ref32 - want) + 1e-5 * abs(want)
        for name, got, w64, w32 in zip(P.TABLES, _tables(eng), P.golden_tables(g, case, "f64", k),
                                       P.golden_tables(g, case, "f32", k)):
            bar = np.abs(w32.astype(np.float64) - w64).max()
            err = np.abs(got.astype(np.float64) - w64).max()
            print("%s step %d %s: device err %.3g, reference f32 err %.3g" % (case, k + 1, name, err, bar))
            assert got.shape == w64.shape and err <= 4 * bar + 1e-5 * np.abs(w64).max(), (case, k, name, err, bar)
            still = np.setdiff1d(np.arange(len(got)), g["%s_rows_%s" % (case, name)])
            assert len(still) and np.array_equal(got[still], g[name + "_0"][still]), (case, k, name)
    assert eng.t == len(g[case + "_users"])
    for name in P.TABLES:                                     # the gradient buffers are zero again
        assert not eng.G[name].any().item(), name


def test_predict_matches_the_reference(golden):
    """score() after the trained case `bpr_adam`, full rows and the candidates' entries, under the trace's rule: no
    bias"""
    import torch
    g = golden
    eng = _engine(g, P.PREDICT_CASE)
    loss2 = torch.zeros(2, device=eng.P.device)
    for k in range(len(g[P.PREDICT_CASE + "_users"])):
        _feed(eng, _batch(g, P.PREDICT_CASE, k), loss2)
    w64, w32 = g["predict_f64"], g["predict_f32"]
    got = eng.score(g["predict_users"]).cpu().numpy().astype(np.float64)
    assert got.shape == w64.shape
    assert np.abs(got - w64).max() <= 4 * np.abs(w32 - w64).max() + 1e-5 * np.abs(w64).max()
    got_c = np.stack([got[k][c] for k, c in enumerate(g["predict_cand"])])
    c64, c32 = g["predict_cand_f64"], g["predict_cand_f32"]
    assert np.abs(got_c - c64).max() <= 4 * np.abs(c32 - c64).max() + 1e-5 * np.abs(c64).max()


def _toy(U, I, d, seed, scale):
    rs = np.random.RandomState(seed)
    tabs = [(scale * rs.randn(*shape)).astype(np.float32) for shape in ((U, d), (I, d), (I,))]
    tr = (np.arange(U + 1, dtype=np.int64), (np.arange(U) % I).astype(np.int32))       # one item each
    trust = (np.arange(U + 1, dtype=np.int64), ((np.arange(U) + 1) % U).astype(np.int32))
    return tabs, tr, trust


def _random_batch(rs, U, I, B):
    users = rs.randint(U, size=B).astype(np.int32)
    items, social, neg = (rs.randint(I, size=B).astype(np.int32) for _ in range(3))
    suk = rs.randint(1, 6, size=B).astype(np.float32)
    social[0] = items[0]                                      # i = k inside a slot
    if B > 1:
        neg[1] = social[1]                                    # k = j inside a slot
    if B > 2:
        items[2] = social[2] = neg[2]                         # all three
    return users, items, social, neg, suk


def _against_restatement(d, sizes, loss, learner="gd", seed=0):
    """the engine and the float64 restatement fed the same batches: loss and tables within 1e-5 max|want| after every
    step (fp32 storage of O(0.1) tables and fp32 loss terms).  Plain gradient descent is linear in the gradient, so a
    wrong or missing term of any gradient shows at its full size"""
    import torch
    from neurec_amd.sbpr import SBPREngine
    U, I = 23, 31
    scale = 0.5 if d == 1 else 0.3 if d <= 20 else 0.1
    tabs, tr, trust = _toy(U, I, d, d, scale)
    eng = SBPREngine(*tabs, tr, trust, LR, 0.01, max(sizes), loss=loss, learner=learner)
    st = P.State(*tabs, learner=learner, lr=LR)
    rs = np.random.RandomState(1000 * d + sizes[0] + seed)
    loss2 = torch.zeros(2, device=eng.P.device)
    for k, B in enumerate(sizes):
        batch = _random_batch(rs, U, I, B)
        got = _feed(eng, batch, loss2)
        want = P.step(st, *batch, loss, 0.01)
        assert abs(got - want) <= 1e-5 * abs(want), (d, B, got, want)
        for name, t in zip(P.TABLES, _tables(eng)):
            err = np.abs(t - st.var[name]).max()
            assert err <= 1e-5 * np.abs(st.var[name]).max(), (name, d, B, err)
    return eng


@pytest.mark.parametrize("d", [1, 16, 50, 128])
@pytest.mark.parametrize("loss", ["bpr", "hinge", "square"])
def test_widths_and_batch_sizes_against_the_restatement(d, loss):
    """every lane layout crossed with B = 1, B = 33 twice, and 64 followed by a short last batch of 7: 23 users and 31
    items, so rows repeat in every role; slots with i = k, with k = j and with i = k = j"""
    for sizes in ((1, 1), (33, 33), (64, 7)):
        _against_restatement(d, sizes, loss)


def test_momentum_against_the_restatement():
    """the other learner that is linear in the gradient, over three steps: its accumulator carries from step to step.
    (adam, adagrad and rmsprop divide by a root of squared gradients that starts at 1e-8 or less, which multiplies the
    fp32 rounding of a near-zero gradient entry by up to lr / 1e-4: they are checked on the reference's trace, under
    its own f32-to-f64 distance)"""
    _against_restatement(16, (33, 33, 5), "bpr", learner="momentum")


def _adam_run():
    import torch
    from neurec_amd.sbpr import SBPREngine
    tabs, tr, trust = _toy(23, 31, 50, 9, 0.1)
    eng = SBPREngine(*tabs, tr, trust, 0.01, 0.01, 64, loss="bpr", learner="adam")
    rs = np.random.RandomState(77)
    loss2 = torch.zeros(2, device=eng.P.device)
    losses = [_feed(eng, _random_batch(rs, 23, 31, B), loss2) for B in (64, 64, 7)]
    return eng, losses


def test_an_empty_batch_moves_nothing_and_reruns_are_bit_identical():
    import torch
    eng, losses = _adam_run()
    again, losses2 = _adam_run()
    assert losses == losses2 and np.all(np.isfinite(losses))
    for a, b, t0 in zip(_tables(eng), _tables(again), _toy(23, 31, 50, 9, 0.1)[0]):
        assert np.array_equal(a, b) and not np.array_equal(a, t0)
    before, t = _tables(eng), eng.t
    loss2 = torch.ones(2, device=eng.P.device)
    empty = _dev(eng, *(np.zeros(0, np.int32),) * 4, np.zeros(0, np.float32))
    eng.step(*empty, loss2)
    assert loss2.tolist() == [0.0, 0.0] and eng.t == t == 3
    for a, b in zip(before, _tables(eng)):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="larger than max_batch"):
        eng.step(*_dev(eng, *(np.zeros(65, np.int32),) * 4, np.ones(65, np.float32)), loss2)


def test_train_epoch_runs_the_stream_with_a_short_last_batch(golden):
    """the epoch's steps against the restatement fed the same stream in batches of 64 (momentum: linear in the
    gradient); the instance count is no multiple of 64"""
    g = golden
    eng = _engine(g, "bpr_momentum", seed=5)
    total, n = eng.train_epoch(0, 64)
    assert n == len(g["epoch_users"]) and eng.t == (n + 63) // 64 and n % 64 != 0 and np.isfinite(total)
    st = P.State(g["P_0"], g["Q_0"], g["b_0"], learner="momentum", lr=float(g["learning_rate"]))
    fields = _epoch(_engine(g, "bpr_momentum", seed=5), 0)
    want = sum(P.step(st, *(f[lo:lo + 64] for f in fields), "bpr", float(g["reg_mf"])) for lo in range(0, n, 64))
    assert abs(total - want) <= 1e-5 * abs(want)
    for name, t in zip(P.TABLES, _tables(eng)):
        assert np.abs(t - st.var[name]).max() <= 1e-5 * np.abs(st.var[name]).max()


# ------------------------------------------------------------------ drop-in
def test_sbpr_config_drops_in(tmp_path):
    """NeuRec.properties + conf/SBPR.properties (the reference's values, at learning_rate 0.01) + a trust file with
    unknown ids: two epochs through neurec_amd.main; the reference's log lines from epoch 0; the logged loss finite;
    predict() in both modes = P Q^T of the engine's tables, without the bias"""
    from neurec_amd.main import main
    from test_fpmc_gpu import _write_dataset
    _write_dataset(str(tmp_path))
    rs = np.random.RandomState(4)
    trust = os.path.join(str(tmp_path), "dataset", "toy.uu")
    with open(trust, "w") as f:
        for u in range(120):
            if u % 9 == 0:
                continue
            for v in rs.choice(120, 3, replace=False):
                f.write("%d\t%d\n" % (u + 7, v + 7))
        f.write("7\t5000\n5001\t8\n")
    path = defaults.write_default_configs(str(tmp_path), overrides={
        "data.input.path": os.path.join(str(tmp_path), "dataset"), "data.input.dataset": "toy",
        "test_batch_size": "64"}, model_overrides={"SBPR": {"learning_rate": "0.01", "social_file": trust}})
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        model = main(argv=["--recommender=SBPR", "--num_epochs=2"], properties=path)
    finally:
        os.chdir(cwd)
    eng = model.engine
    assert eng.d == 16 and eng.t == 2 * ((eng.n_instances + 511) // 512) and eng.n_instances > 0
    assert model.social_matrix.nnz == eng.s_indices.numel() > 300
    folder = os.path.join(str(tmp_path), "log", "toy", "SBPR")
    files = os.listdir(folder)
    assert len(files) == 1
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "SBPR's hyperparameters:" in text
    kinds = re.findall(r"(metrics:\t|\[iter \d+ : loss|epoch \d+:\t)", text)
    assert kinds == ["metrics:\t", "[iter 0 : loss", "epoch 0:\t", "[iter 1 : loss", "epoch 1:\t"], kinds
    logged = [float(x) for x in re.findall(r"\[iter \d+ : loss : ([-0-9.naif]+),", text)]
    assert len(logged) == 2 and np.all(np.isfinite(logged)) and np.all(np.isfinite(model.epoch_losses))
    assert model.epoch_losses[1] < model.epoch_losses[0]
    Pm, Q, b = (t.astype(np.float64) for t in _tables(eng))
    assert np.abs(b).max() > 0
    full = model.predict([0, 5, 9], None)
    want = Pm[[0, 5, 9]] @ Q.T
    assert full.shape == (3, model.num_items) and np.abs(full - want).max() <= 1e-5 * np.abs(want).max()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])
    assert np.array_equal(cand[1], full[1][[7]])
