"""APR without a GPU: the numpy restatement (tests/apr_restatement.py) against the reference class's own float64 trace
(tests/golden/tfgraph_apr.npz) and against torch autograd, and the host-side pieces of the port — the recommender's
registration, the defaults row, the build list, the header's limits, the mode table and the refusals."""
import configparser
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import apr_restatement as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_apr")


def _tight(got, want, what, ulps=8):
    """within `ulps` float64 ulps of max(1, the largest value): test_jca_cpu._tight's bound — the two float64 runs
    differ by the order of their sums"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max(initial=0)
    bar = ulps * EPS64 * max(1.0, np.abs(want).max(initial=0))
    print("%s: err %.3g (%.1f ulps of the scale)" % (what, err, err / (bar / ulps)))
    assert got.shape == want.shape and err <= bar, (what, err, bar)


def case_mode(case):
    """(adversarial, with_reg, dense) of a golden case.  Outside the shipped loop the class's graph holds
    reg * l2_loss(P, Q) even at reg = 0, so the shim gives the tables its DENSE kernels there; at reg = 0 the rows
    outside the batch have a zero gradient and the dense and the sparse form differ in how Adam's moments round"""
    adv = A.CASES[case][0]
    return adv in ("grad", "random"), adv != "shipped", adv != "shipped"


@pytest.mark.parametrize("case", sorted(A.CASES))
def test_restatement_reproduces_the_float64_trace(golden, case):
    """every table after every step, Delta on the batch's rows and both losses, within 8 float64 ulps of
    max(1, largest value).  `random_adam` replays the recorded Delta."""
    g = golden
    adv, learner, d, reg, reg_adv, eps = A.CASES[case]
    adversarial, with_reg, dense = case_mode(case)
    P0, Q0 = A.golden_tables(g, case, "f64", -1)
    assert P0.shape == (157, d) and Q0.shape == (131, d)
    st = A.State(P0, Q0, learner=learner, lr=float(g["learning_rate"]))
    for s in range(A.STEPS):
        users, pos, neg = (g["%s_%s" % (case, f)][s] for f in ("users", "pos", "neg"))
        assert len(users) == A.BATCH and all(A.edge_patterns(users, pos, neg).values())
        delta = A.golden_delta(g, case, "f64", s, (P0.shape, Q0.shape)) if adv == "random" else None
        loss, opt, dP, dQ = A.step(st, users, pos, neg, reg, reg_adv, eps, adversarial, with_reg, delta, dense=dense)
        _tight(loss, g[case + "_f64_loss"][s], "%s step %d loss" % (case, s))
        if adv != "shipped":
            _tight(opt, g[case + "_f64_opt_loss"][s], "%s step %d opt_loss" % (case, s))
        if adv == "grad":
            wP, wQ = A.golden_delta(g, case, "f64", s, (P0.shape, Q0.shape))
            _tight(dP, wP, "%s step %d Delta_P" % (case, s))
            _tight(dQ, wQ, "%s step %d Delta_Q" % (case, s))
            rows = g["%s_drows_P_%d" % (case, s)]
            np.testing.assert_allclose(np.sqrt((dP[rows] ** 2).sum(axis=1)), eps, rtol=1e-12)
        wP, wQ = A.golden_tables(g, case, "f64", s)
        _tight(st.P, wP, "%s step %d P" % (case, s))
        _tight(st.Q, wQ, "%s step %d Q" % (case, s))


def test_shipped_loop_ignores_the_adversarial_keys(golden):
    """`shipped_adam` ran with reg = 0.05: the restatement of `loss` alone reproduces it (above), and rows outside the
    batches never move"""
    g = golden
    assert not bool(g["shipped_adam_every_row_moved"]) and bool(g["plain_reg_adam_every_row_moved"])
    rows = set()
    for s in range(A.STEPS):
        rows |= set(g["shipped_adam_users"][s].tolist())
    assert set(g["shipped_adam_rows_P"].tolist()) == rows


def test_random_trace_holds_truncated_draws(golden):
    g = golden
    eps = A.CASES["random_adam"][5]
    for s in range(A.STEPS):
        for t in "PQ":
            draw = g["random_adam_draw_%s_%d" % (t, s)].astype(np.float64)
            assert np.abs(draw).max() <= 0.02 + 1e-9
            _tight(A.normalise(draw, eps), g["random_adam_f64_delta_%s_%d" % (t, s)], "draw %s %d" % (t, s))


def test_restatement_epoch_of_the_shipped_class(golden):
    """the recorded train_model() epoch: per-step losses, the logged figure and the end tables"""
    g = golden
    P0, Q0 = A.golden_tables(g, "epoch", "f64", -1)
    st = A.State(P0, Q0, learner="adam", lr=float(g["learning_rate"]))
    at, losses = 0, []
    for n in g["epoch_sizes"]:
        b = [g["epoch_" + f][at:at + n] for f in ("users", "pos", "neg")]
        losses.append(A.step(st, *b, reg=0.05, adversarial=False, with_reg=False)[0])
        at += n
    _tight(np.asarray(losses), g["epoch_f64_losses"], "epoch losses")
    assert abs(sum(losses) / len(losses) - float(g["epoch_f64_logged"])) <= 1e-6 * abs(sum(losses) / len(losses))
    wP, wQ = A.golden_tables(g, "epoch", "f64", 0)
    _tight(st.P, wP, "epoch end P")
    _tight(st.Q, wQ, "epoch end Q")
    users = g["predict_users"]
    _tight(st.P[users] @ st.Q.T, g["predict_f64"], "predict")
    cand = g["predict_cand"]
    _tight(np.stack([(st.P[u] @ st.Q[c].T) for u, c in zip(users, cand)]), g["predict_cand_f64"], "predict, candidates")


@pytest.mark.parametrize("adversarial,reg", [(True, 0.05), (True, 0.0), (False, 0.05)])
def test_restatement_gradient_equals_autograd(adversarial, reg):
    """G of the restatement = torch autograd of opt_loss with Delta detached, float64, to the same bound"""
    import torch
    rs = np.random.RandomState(5)
    U, I, d, B = 23, 19, 7, 40
    P, Q = 0.3 * rs.randn(U, d), 0.3 * rs.randn(I, d)
    u, i, j = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, I, B)
    j[3] = i[3]                                                # a pair with i == j
    reg_adv, eps = 0.7, 0.4
    loss, opt, GP, GQ, dP, dQ = A.gradients(P, Q, u, i, j, reg, reg_adv, eps, adversarial, True)
    tP, tQ = torch.tensor(P, requires_grad=True), torch.tensor(Q, requires_grad=True)
    tu, ti, tj = (torch.as_tensor(x, dtype=torch.int64) for x in (u, i, j))

    def plain(p, qi, qj):
        return torch.nn.functional.softplus(-((p * qi).sum(1) - (p * qj).sum(1))).sum()
    tl = plain(tP[tu], tQ[ti], tQ[tj])
    total = tl + reg * ((tP * tP).sum() / 2 + (tQ * tQ).sum() / 2)
    if adversarial:
        gP, gQ = torch.autograd.grad(tl, [tP, tQ], retain_graph=True)

        def norm(x):
            return (x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12)) * eps).detach()
        DP, DQ = norm(gP), norm(gQ)
        _tight(dP, DP.numpy(), "Delta_P")
        _tight(dQ, DQ.numpy(), "Delta_Q")
        total = total + reg_adv * plain(tP[tu] + DP[tu], tQ[ti] + DQ[ti], tQ[tj] + DQ[tj])
    wP, wQ = torch.autograd.grad(total, [tP, tQ])
    _tight(loss, tl.item(), "loss")
    _tight(opt, total.item(), "opt_loss")
    _tight(GP, wP.numpy(), "G_P")
    _tight(GQ, wQ.numpy(), "G_Q")


def test_float32_restatement_stays_in_float32():
    rs = np.random.RandomState(2)
    P, Q = (0.1 * rs.randn(9, 4)).astype(np.float32), (0.1 * rs.randn(8, 4)).astype(np.float32)
    for learner in A.LEARNERS:
        st = A.State(P, Q, learner=learner, dtype=np.float32)
        loss, opt, dP, dQ = A.step(st, [1, 1, 2], [0, 3, 3], [3, 5, 0], reg=0.05)
        assert st.P.dtype == st.Q.dtype == dP.dtype == np.float32 and np.asarray(loss).dtype == np.float32
        assert np.isfinite(st.P).all() and not np.array_equal(st.P, P)


# ------------------------------------------------------------------ the port's host side
def test_find_recommender_returns_the_class():
    from neurec_amd.main import find_recommender
    cls = find_recommender("APR")
    assert cls.__name__ == "APR" and cls.__module__ == "neurec_amd.model.general_recommender.APR"
    keys = re.findall(r'conf\["(\w+)"\]', __import__("inspect").getsource(cls.__init__))
    assert keys[:14] == ["learning_rate", "embedding_size", "learner", "epochs", "eps", "adv", "adver", "adv_epoch",
                         "reg", "reg_adv", "batch_size", "init_method", "stddev", "verbose"]         # APR.py:18-31


def test_the_defaults_row_equals_the_properties_file(tmp_path):
    from neurec_amd import defaults
    ref = configparser.ConfigParser()
    ref.optionxform = str
    assert ref.read(os.path.join(GOLDEN, "neurec_conf", "conf", "APR.properties"))
    want = dict(ref["hyperparameters"])
    assert list(want) == ["epochs", "batch_size", "embedding_size", "reg", "reg_adv", "learning_rate", "learner",
                          "adv_epoch", "adv", "eps", "adver", "init_method", "stddev", "verbose"]
    assert dict(defaults.MODELS["APR"]) == want and [k for k, _ in defaults.MODELS["APR"]] == list(want)
    path = defaults.write_default_configs(str(tmp_path))
    from neurec_amd.util.configurator import Configurator
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        conf = Configurator(path, default_section="hyperparameters", argv=["--recommender=APR"])
    finally:
        os.chdir(cwd)
    assert (conf["epochs"], conf["embedding_size"], conf["reg"], conf["reg_adv"], conf["adv"], conf["eps"],
            conf["adver"], conf["adv_epoch"]) == (30, 64, 0, 1, "grad", 0.5, 1, 0)


def test_the_source_is_in_the_build_list():
    from neurec_amd import build
    assert "apr.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "apr.hip"))
    from neurec_amd import _lib
    assert "nrhip_apr_step" in _lib.EXPORTED


def test_header_limits_match_the_engine():
    from neurec_amd import apr
    with open(os.path.join(ROOT, "include", "neurec_hip.h")) as fh:
        header = fh.read()
    macros = dict(re.findall(r"#define NRHIP_APR_(\w+) (\(1 << \d+\)|\d+)", header))
    assert eval(macros["MAX_D"]) == apr.MAX_D == 128
    assert eval(macros["MAX_BATCH"]) == apr.MAX_BATCH == 1 << 24
    assert eval(macros["L2_BLOCKS"]) == apr.L2_BLOCKS == 256
    text = re.search(r"/\* ---- APR .*?\*/", header, re.S).group(0)
    for words in ("n_users + n_items < 2^31", "NRHIP_APR_MAX_BATCH", "NRHIP_ERR_UNSUPPORTED", "bit-identical"):
        assert words in text, words


def test_argument_struct_matches_the_header():
    """the ctypes struct names the header's fields in the header's order"""
    from neurec_amd import _lib
    with open(os.path.join(ROOT, "include", "neurec_hip.h")) as fh:
        body = re.search(r"typedef struct nrhip_apr_step_args \{(.*?)\} nrhip_apr_step_args;", fh.read(), re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        for piece in decl.split(",") if decl else ():
            name = re.search(r"(\w+)$", piece.strip()).group(1)
            names.append(name[2:] if name.startswith("d_") else name)
    assert names == [n for n, _ in _lib.AprStepArgs._fields_], names


@pytest.mark.parametrize("switch", [False, True])
@pytest.mark.parametrize("adver", [0, 1])
@pytest.mark.parametrize("adv_epoch", [0, 1, 7])
def test_mode_table(adv_epoch, adver, switch):
    """which of 4 epochs perturb: adver truthy and epoch > adv_epoch; none in the loop as shipped"""
    from neurec_amd.apr import adversarial_epoch
    got = [e for e in range(1, 5) if adversarial_epoch(e, adver, adv_epoch, switch)]
    want = [] if (switch or not adver) else {0: [1, 2, 3, 4], 1: [2, 3, 4], 7: []}[adv_epoch]
    assert got == want == A.adversarial_epochs(4, adver, adv_epoch, switch)


def test_engine_refusals_before_any_device_work():
    from neurec_amd.apr import APREngine
    P, Q = np.zeros((5, 4), np.float32), np.zeros((6, 4), np.float32)
    with pytest.raises(ValueError, match="adv='fgsm' is not supported"):
        APREngine(P, Q, 0.01, 0.0, 1.0, 0.5, 8, adv="fgsm")
    with pytest.raises(ValueError, match="please select a suitable optimizer"):
        APREngine(P, Q, 0.01, 0.0, 1.0, 0.5, 8, learner="lbfgs")
    with pytest.raises(NotImplementedError, match="embedding_size=129 is not supported \\(1 to 128\\)"):
        APREngine(np.zeros((5, 129), np.float32), np.zeros((6, 129), np.float32), 0.01, 0.0, 1.0, 0.5, 8)
    with pytest.raises(NotImplementedError, match="1 to 128"):
        APREngine(np.zeros((5, 0), np.float32), np.zeros((6, 0), np.float32), 0.01, 0.0, 1.0, 0.5, 8)
    with pytest.raises(ValueError, match="embedding_size"):
        APREngine(P, np.zeros((6, 5), np.float32), 0.01, 0.0, 1.0, 0.5, 8)
    with pytest.raises(ValueError, match="max_batch"):
        APREngine(P, Q, 0.01, 0.0, 1.0, 0.5, (1 << 24) + 1)
