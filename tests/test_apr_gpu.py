"""APR on the GPU (csrc/apr.hip through neurec_amd/apr.py): every step of the reference class's trace, the width
ladder, the two branches of the normalisation, a hub run, the batch sizes, ids outside the tables, determinism, the
`random` mode's draws, and the drop-in run through neurec_amd.main with the loop as shipped replayed."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import apr_restatement as A

pytestmark = pytest.mark.gpu

SORT_ONE_WORKGROUP = 16384          # keys nrhip_sort_u64 sorts in one workgroup's LDS
LR = 0.05                           # gd steps of the edge tests: a gradient term of 0.1 moves a table by 5e-3


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_apr")


def _dev(eng, *arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(eng.P.device) for a in arrays)


def _tables(eng):
    return eng.P.cpu().numpy(), eng.Q.cpu().numpy()


def _whole(shape, rows, vals):
    out = np.zeros(shape, np.float64)
    out[rows.cpu().numpy()] = vals.cpu().numpy()
    return out


def _deltas(eng):
    rp, dp, rq, dq = eng.deltas()
    return _whole(tuple(eng.P.shape), rp, dp), _whole(tuple(eng.Q.shape), rq, dq)


def _toy_tables(d, seed, U=157, I=131, scale=0.1):
    rs = np.random.RandomState(seed)
    return (scale * rs.randn(U, d)).astype(np.float32), (scale * rs.randn(I, d)).astype(np.float32)


def _rule(got, w64, w32, what):
    """the project's rule: the device's distance to the float64 value is at most 4 x the float32 twin's own distance
    plus 1e-5 max|want|"""
    got, w64, w32 = (np.asarray(x, np.float64) for x in (got, w64, w32))
    err, bar = np.abs(got - w64).max(initial=0), np.abs(w32 - w64).max(initial=0)
    print("%s: device err %.3g, float32 twin err %.3g" % (what, err, bar))
    assert got.shape == w64.shape and err <= 4 * bar + 1e-5 * np.abs(w64).max(initial=0), (what, err, bar)


def _golden_engine(g, case, reg=None, **kw):
    from neurec_amd.apr import APREngine
    adv, learner, d, reg0, reg_adv, eps = A.CASES[case]
    return APREngine(g[case + "_P_0"], g[case + "_Q_0"], float(g["learning_rate"]), reg0 if reg is None else reg, reg_adv,
                     eps, A.BATCH, adv="random" if adv == "random" else "grad", learner=learner, **kw)


def _run_case(g, case, reg=None, check=True):
    import torch
    adv = A.CASES[case][0]
    adversarial, with_reg = adv in ("grad", "random"), adv != "shipped"
    eng = _golden_engine(g, case, reg)
    loss2 = torch.zeros(2, device=eng.P.device)
    shapes = (tuple(eng.P.shape), tuple(eng.Q.shape))
    for s in range(A.STEPS):
        batch = _dev(eng, *(g["%s_%s" % (case, f)][s] for f in ("users", "pos", "neg")))
        given = None
        if adv == "random":                                    # the recorded Delta of the float32 run's draws
            given = tuple(torch.from_numpy(np.ascontiguousarray(g[k % (case, s)])).to(eng.P.device)
                          for k in ("%s_drows_P_%d", "%s_f32_delta_P_%d", "%s_drows_Q_%d", "%s_f32_delta_Q_%d"))
        eng.step(*batch, loss2, adversarial=adversarial, with_reg=with_reg, delta_given=given)
        if not check:
            continue
        got = loss2.cpu().numpy().astype(np.float64)
        what = "%s step %d " % (case, s + 1)
        _rule(got[0], g[case + "_f64_loss"][s], g[case + "_f32_loss"][s], what + "loss")
        if adv != "shipped":
            _rule(got.sum(), g[case + "_f64_opt_loss"][s], g[case + "_f32_opt_loss"][s], what + "opt_loss")
        else:
            assert got[1] == 0.0
        if adversarial:
            for name, d_got, w64, w32 in zip("PQ", _deltas(eng), A.golden_delta(g, case, "f64", s, shapes),
                                             A.golden_delta(g, case, "f32", s, shapes)):
                _rule(d_got, w64, w32, what + "Delta_" + name)
        for name, t_got, w64, w32, t0 in zip("PQ", _tables(eng), A.golden_tables(g, case, "f64", s),
                                             A.golden_tables(g, case, "f32", s), (g[case + "_P_0"], g[case + "_Q_0"])):
            _rule(t_got, w64, w32, what + name)
            if eng.learner != "adam":                          # the row learners leave the other rows alone, in bits
                still = np.setdiff1d(np.arange(len(t_got)), g["%s_rows_%s" % (case, name)])
                assert np.array_equal(t_got[still], t0[still]), (case, s, name)
                assert len(still) or bool(g[case + "_every_row_moved"])
        assert not eng.GP.any().item() and not eng.GQ.any().item()
        assert eng.flagP is None or (not eng.flagP.any().item() and not eng.flagQ.any().item())
    return eng


@pytest.mark.parametrize("case", sorted(A.CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Both losses, Delta (from deltas()) and both tables after every step against the float64 trace, by the project's
    rule with the reference's own float32 trace as the yardstick.  Under the row learners the rows the trace never
    moves are bit-equal to their initial values; G and the flags are zero again afterwards.  `random_adam` runs with
    delta_given = the recorded Delta."""
    _run_case(golden, case)


def test_shipped_loop_ignores_reg(golden):
    """`shipped_adam` with reg = 0.05 and with reg = 0: the same tables, in bits"""
    import torch
    a, b = _run_case(golden, "shipped_adam", reg=0.05, check=False), _run_case(golden, "shipped_adam", reg=0.0, check=False)
    assert torch.equal(a.P, b.P) and torch.equal(a.Q, b.Q)


def _against_restatement(P0, Q0, batches, reg=0.0, reg_adv=0.5, eps=0.1, learner="gd", adversarial=True, lr=LR,
                         max_batch=None, fed=None):
    """the engine against the restatement in float64, the bound from the restatement's own float32 twin: 4 x its
    float32-to-float64 distance plus 1e-5 max|want| for both losses, Delta and both tables after every step.
    fed: the batches the engine gets when they differ from the restatement's (ids outside the tables)"""
    import torch
    from neurec_amd.apr import APREngine
    eng = APREngine(P0, Q0, lr, reg, reg_adv, eps, max_batch or max(len(b[0]) for b in (fed or batches)),
                    learner=learner)
    s64 = A.State(P0, Q0, learner=learner, lr=lr)
    s32 = A.State(P0, Q0, learner=learner, lr=lr, dtype=np.float32)
    loss2 = torch.zeros(2, device=eng.P.device)
    for k, b in enumerate(batches):
        eng.step(*_dev(eng, *(fed or batches)[k]), loss2, adversarial=adversarial)
        w64 = A.step(s64, *b, reg, reg_adv, eps, adversarial)
        w32 = A.step(s32, *b, reg, reg_adv, eps, adversarial)
        got = loss2.cpu().numpy().astype(np.float64)
        _rule(got[0], w64[0], w32[0], "step %d loss" % k)
        _rule(got.sum(), w64[1], w32[1], "step %d opt_loss" % k)
        if adversarial:
            dP, dQ = _deltas(eng)
            _rule(dP, w64[2], w32[2], "step %d Delta_P" % k)
            _rule(dQ, w64[3], w32[3], "step %d Delta_Q" % k)
        _rule(eng.P.cpu().numpy(), s64.P, s32.P, "step %d P" % k)
        _rule(eng.Q.cpu().numpy(), s64.Q, s32.Q, "step %d Q" % k)
    return eng, s64


def _random_batches(rs, U, I, B, steps=2):
    return [tuple(rs.randint(0, n, B).astype(np.int32) for n in (U, I, I)) for _ in range(steps)]


@pytest.mark.parametrize("d", [1, 16, 17, 32, 33, 64, 65, 128])
def test_width_ladder(d):
    """every lane-group shape of the launch ladder and the widths beside its steps: two gd steps of a batch of 40"""
    P0, Q0 = _toy_tables(d, seed=d)
    _against_restatement(P0, Q0, _random_batches(np.random.RandomState(100 + d), 157, 131, 40))


def test_width_129_is_refused():
    from neurec_amd.apr import APREngine
    P0, Q0 = _toy_tables(129, seed=1)
    with pytest.raises(NotImplementedError, match="1 to 128"):
        APREngine(P0, Q0, LR, 0.0, 1.0, 0.5, 40)


@pytest.mark.parametrize("learner,reg", [("adagrad", 0.0), ("rmsprop", 0.0), ("momentum", 0.05), ("adam", 0.05),
                                         ("rmsprop", 0.05)])
def test_learner_forms(learner, reg):
    """the sparse application at reg = 0 and the dense one at reg != 0, for the learners the trace does not hold"""
    P0, Q0 = _toy_tables(12, seed=3)
    _against_restatement(P0, Q0, _random_batches(np.random.RandomState(7), 157, 131, 40, steps=3), reg=reg,
                         learner=learner, lr=0.01)


def test_zero_norm_branch():
    """one triplet (u, i, i) whose user and item occur nowhere else: Gamma of both rows is exactly zero, so Delta is
    0 * rsqrt(1e-12) = 0, everything stays finite and under gd the two rows do not move"""
    rs = np.random.RandomState(11)
    P0, Q0 = _toy_tables(16, seed=12)
    u, i, j = (rs.randint(1, n, 20).astype(np.int32) for n in (157, 131, 131))
    u[5], i[5], j[5] = 0, 0, 0
    eng, _ = _against_restatement(P0, Q0, [(u, i, j)])
    dP, dQ = _deltas(eng)
    assert not dP[0].any() and not dQ[0].any()
    P1, Q1 = _tables(eng)
    assert np.isfinite(P1).all() and np.isfinite(Q1).all()
    assert np.array_equal(P1[0], P0[0]) and np.array_equal(Q1[0], Q0[0])


def test_epsilon_branch():
    """one triplet planted with x about 25: |Gamma|^2 falls below 1e-12 while staying a normal float32, so Delta is
    eps * Gamma * 1e6, not a vector of norm eps"""
    d, eps = 16, 0.1
    P0, Q0 = _toy_tables(d, seed=13)
    P0[0], Q0[0], Q0[1] = 1.25, 1.25, 0.0                      # x = 16 * 1.25^2 = 25
    u, i, j = np.asarray([0], np.int32), np.asarray([0], np.int32), np.asarray([1], np.int32)
    eng, _ = _against_restatement(P0, Q0, [(u, i, j)], eps=eps)
    s = -1.0 / (1.0 + np.exp(25.0))
    gamma_p = s * (Q0[0].astype(np.float64) - Q0[1])
    n2 = float((gamma_p ** 2).sum())
    assert np.finfo(np.float32).tiny < n2 < 1e-12
    dP, _ = _deltas(eng)
    want = eps * gamma_p * 1e6
    assert np.abs(dP[0] - want).max() <= 1e-5 * np.abs(want).max()
    assert np.sqrt((dP[0] ** 2).sum()) < 1e-3 * eps


def test_hub_run():
    """300 triplets with one user and one positive item at d = 65: two runs of 300 keys walked by one lane group"""
    rs = np.random.RandomState(17)
    P0, Q0 = _toy_tables(65, seed=18, scale=0.05)
    batches = [(np.full(300, 3, np.int32), np.full(300, 5, np.int32), rs.randint(0, 131, 300).astype(np.int32))
               for _ in range(2)]
    _against_restatement(P0, Q0, batches, lr=0.002)


def test_batch_of_one_and_of_none():
    import torch
    P0, Q0 = _toy_tables(16, seed=19)
    one = tuple(np.asarray([x], np.int32) for x in (4, 9, 2))
    eng, _ = _against_restatement(P0, Q0, [one], max_batch=4)
    before = [t.clone() for t in eng.tables()]
    loss2 = torch.full((2,), 7.0, device=eng.P.device)
    empty = torch.zeros(0, dtype=torch.int32, device=eng.P.device)
    eng.step(empty, empty, empty, loss2)
    assert loss2.tolist() == [0.0, 0.0]
    assert all(torch.equal(a, b) for a, b in zip(eng.tables(), before))
    with pytest.raises(ValueError, match="batch larger than max_batch"):
        eng.step(*_dev(eng, *(np.zeros(5, np.int32),) * 3), loss2)
    with pytest.raises(ValueError, match="same length"):
        eng.step(*_dev(eng, np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(1, np.int32)), loss2)


def test_one_batch_beyond_the_one_workgroup_sort():
    """6,000 triplets at d = 8: 18,000 keys, past the 16,384 that nrhip_sort_u64 sorts in one workgroup"""
    B, U, I = 6000, 3000, 2500
    assert 3 * B > SORT_ONE_WORKGROUP
    P0, Q0 = _toy_tables(8, seed=23, U=U, I=I)
    _against_restatement(P0, Q0, _random_batches(np.random.RandomState(29), U, I, B))


@pytest.mark.parametrize("adversarial", [True, False])
def test_ids_outside_the_tables_take_no_part(adversarial):
    """a triplet with an id outside its table takes no part in either pass: the result equals the batch without it,
    bit for bit"""
    import torch
    from neurec_amd.apr import APREngine
    rs = np.random.RandomState(31)
    P0, Q0 = _toy_tables(17, seed=37)
    (u, i, j), = _random_batches(rs, 157, 131, 30, steps=1)
    fu, fi, fj = (np.insert(x, [0, 7, 7, 30], bad) for x, bad in ((u, [157, 3, -1, 4]), (i, [2, 131, 5, 6]),
                                                                   (j, [1, 2, 3, -5])))
    ends = []
    for batch in ((fu, fi, fj), (u, i, j)):
        eng = APREngine(P0, Q0, LR, 0.0, 0.5, 0.1, 40, learner="gd")
        loss2 = torch.zeros(2, device=eng.P.device)
        eng.step(*_dev(eng, *batch), loss2, adversarial=adversarial)
        ends.append((eng.P.clone(), eng.Q.clone(), loss2.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*ends))
    assert not torch.equal(ends[0][0], torch.from_numpy(P0).to(ends[0][0].device))


@pytest.mark.parametrize("adv", ["grad", "random"])
def test_two_engines_end_bit_identical(adv):
    import torch
    from neurec_amd.apr import APREngine
    P0, Q0 = _toy_tables(33, seed=41)
    batches = _random_batches(np.random.RandomState(43), 157, 131, 48, steps=3)
    ends = []
    for _ in range(2):
        eng = APREngine(P0, Q0, 0.01, 0.0, 1.0, 0.5, 48, adv=adv, learner="adam", seed=99)
        loss2 = torch.zeros(2, device=eng.P.device)
        for b in batches:
            eng.step(*_dev(eng, *b), loss2)
        ends.append((eng.P, eng.Q, loss2))
    assert all(torch.equal(a, b) for a, b in zip(*ends))


def test_random_delta_rows():
    """the drawn Delta: every row of norm eps, other draws at the next step and for another seed, the mean component
    of 20,000 rows within 5 standard errors of 0, and a step fed deltas() of a drawn step reproduces it in bits"""
    import torch
    from neurec_amd.apr import APREngine
    d, eps, N = 16, 0.5, 20000
    P0, Q0 = _toy_tables(d, seed=47, U=N, I=300)
    users = np.arange(N, dtype=np.int32)
    rs = np.random.RandomState(53)
    pos, neg = rs.randint(0, 300, N).astype(np.int32), rs.randint(0, 300, N).astype(np.int32)

    def engine(seed=2018):
        return APREngine(P0, Q0, 0.01, 0.0, 1.0, eps, N, adv="random", learner="gd", seed=seed)
    eng = engine()
    loss2 = torch.zeros(2, device=eng.P.device)
    eng.step(*_dev(eng, users, pos, neg), loss2)
    rp, dp, rq, dq = first = eng.deltas()
    assert rp.cpu().numpy().tolist() == users.tolist()
    for rows in (dp, dq):
        norms = rows.double().norm(dim=1).cpu().numpy()
        assert np.abs(norms - eps).max() <= 1e-6 * eps, np.abs(norms - eps).max()
    # a component of a uniformly directed vector of norm eps in d dimensions has mean 0 and variance eps^2 / d: the mean
    # of n of them has the standard error (eps / sqrt(d)) / sqrt(n)
    n = dp.numel()
    se = eps / np.sqrt(d) / np.sqrt(n)
    mean = float(dp.double().mean().item())
    print("mean component %.3g, standard error %.3g" % (mean, se))
    assert n == N * d and abs(mean) <= 5 * se
    end = (eng.P.clone(), eng.Q.clone(), loss2.clone())
    eng.step(*_dev(eng, users, pos, neg), loss2)
    assert not torch.equal(eng.deltas()[1], dp)                                       # another step, other draws
    other = engine(seed=7)
    other.step(*_dev(other, users, pos, neg), loss2)
    assert not torch.equal(other.deltas()[1], dp)
    again = engine(seed=123)
    again.step(*_dev(again, users, pos, neg), loss2, delta_given=first)
    assert torch.equal(again.P, end[0]) and torch.equal(again.Q, end[1]) and torch.equal(loss2, end[2])
    assert all(torch.equal(a, b) for a, b in zip(again.deltas(), first))


def test_deltas_needs_an_adversarial_step():
    import torch
    from neurec_amd.apr import APREngine
    P0, Q0 = _toy_tables(4, seed=59)
    eng = APREngine(P0, Q0, LR, 0.0, 1.0, 0.5, 4)
    with pytest.raises(ValueError, match="not adversarial"):
        eng.deltas()
    eng.step(*_dev(eng, [1], [2], [3]), torch.zeros(2, device=eng.P.device), adversarial=False)
    with pytest.raises(ValueError, match="not adversarial"):
        eng.deltas()


# ------------------------------------------------------------------ the plugin
def test_apr_config_drops_in(tmp_path):
    """NeuRec.properties + conf/APR.properties on ml-100k through neurec_amd.main, two epochs with adv_epoch=1: the
    first epoch plain, the second adversarial; the reference's log lines, the mode line, finite metrics, predict()"""
    from test_gru4rec_gpu import _run
    model = _run(tmp_path, ["--recommender=APR", "--epochs=2", "--adv_epoch=1", "--embedding_size=16"])
    assert [model.is_adversarial(e) for e in (1, 2)] == [False, True]
    eng = model.engine
    assert (eng.d, eng.max_batch, eng.adv, eng.learner, eng.reg, eng.reg_adv, eng.eps) == (16, 512, "grad", "adam", 0.0,
                                                                                          1.0, 0.5)
    assert eng.t == 2 * -(-model.dataset.train_matrix.nnz // 512)
    eng.deltas()                                               # the last step was adversarial
    folder = os.path.join(str(tmp_path), "log", "ml-100k", "APR")
    (name,) = os.listdir(folder)
    with open(os.path.join(folder, name)) as f:
        text = f.read()
    assert "APR's hyperparameters:" in text
    assert "reference_train_loop=False (default)" in text and "APR.py:122" in text
    for e in (1, 2):
        assert re.search(r"\[iter %d : loss : [0-9.]+, time: [0-9.]+\]" % e, text)
        shown = np.asarray([float(x) for x in re.findall(r"epoch %d:\t(.+)" % e, text)[0].split()])
        assert np.all(np.isfinite(shown)) and shown.max() > 0
    full = model.predict([0, 5, 9], None)
    assert tuple(full.shape) == (3, model.num_items) and np.isfinite(full).all()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])


def test_plugin_replays_the_shipped_epoch(golden, tmp_path, monkeypatch):
    """reference_train_loop=True with the recorded batches replayed: the end tables and the logged loss of the
    reference class's own train_model() epoch (reg = 0.05 in its conf, without effect), by the project's rule"""
    import torch
    from oracle import ref_models as rm
    import scipy.sparse as sp
    from neurec_amd.model.general_recommender import APR as plugin
    g = golden
    R = sp.csr_matrix((np.ones(len(g["indices"]), np.float32), g["indices"], g["indptr"]), shape=tuple(g["shape"]))
    sizes = g["epoch_sizes"]
    cuts = np.concatenate([[0], np.cumsum(sizes)])

    class Replay:
        def __init__(self, dataset, neg_num=1, batch_size=1024, shuffle=True, as_tensors=False):
            assert as_tensors and batch_size == 64 and neg_num == 1

        def __len__(self):
            return len(sizes)

        def __iter__(self):
            for a, b in zip(cuts[:-1], cuts[1:]):
                yield tuple(torch.from_numpy(g["epoch_" + f][a:b].astype(np.int32)).cuda() for f in ("users", "pos", "neg"))

    monkeypatch.setattr(plugin, "PairwiseSampler", Replay)
    monkeypatch.chdir(tmp_path)
    conf = rm.Conf(rm.NEUREC_DEFAULTS)
    conf.update(recommender="APR", epochs=1, batch_size=64, embedding_size=16, reg=0.05, reg_adv=1.0,
                learning_rate=float(g["learning_rate"]), learner="adam", adv_epoch=0, adv="grad", eps=0.5, adver=1,
                init_method="tnormal", stddev=0.01, verbose=5, reference_train_loop=True)
    model = plugin.APR(None, rm.Dataset(R, test=R), conf)
    model.build_graph()
    model.engine.P.copy_(torch.from_numpy(g["epoch_P_0"]))
    model.engine.Q.copy_(torch.from_numpy(g["epoch_Q_0"]))
    model.train_model()
    assert model.engine.t == len(sizes) and not model.is_adversarial(1)
    for name, got, w64, w32 in zip("PQ", _tables(model.engine), A.golden_tables(g, "epoch", "f64", 0),
                                   A.golden_tables(g, "epoch", "f32", 0)):
        _rule(got, w64, w32, "epoch end " + name)
    (name,) = os.listdir(os.path.join("log", "golden", "APR"))
    with open(os.path.join("log", "golden", "APR", name)) as f:
        text = f.read()
    assert "reference_train_loop=True" in text
    logged = float(re.search(r"\[iter 1 : loss : ([0-9.]+),", text).group(1))
    w64, w32 = float(g["epoch_f64_logged"]), float(g["epoch_f32_logged"])
    # the line prints %f: six decimals of either figure
    assert abs(logged - w64) <= 4 * abs(w32 - w64) + 1e-5 * abs(w64) + 1e-6
    users = g["predict_users"]
    _rule(model.predict(users.tolist(), None), g["predict_f64"], g["predict_f32"], "predict")
    cand = model.predict(users.tolist(), g["predict_cand"].tolist())
    _rule(np.stack(cand), g["predict_cand_f64"], g["predict_cand_f32"], "predict, candidates")
