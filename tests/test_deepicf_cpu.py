"""DeepICF without a GPU: the float64 restatement the GPU tests lean on (tests/deepicf_restatement.py, hand-written
gradients) against the reference class's own float64 trace — every step, every variable, the moving statistics and the
losses, the recorded epoch and predict() —, once against torch autograd, and the properties the golden steps were
chosen for.  The restatement carries each of nine deliberate mistakes as a `variant`; the trace tells every one from the
model."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import fism_restatement as F
import deepicf_restatement as D

STEP_CASES = ("default", "prod_nobn", "odd", "adagrad", "rmsprop", "saturated", "single")


@pytest.fixture(scope="module")
def golden():
    return D.load_trace(load_golden)


def make_state(g, case):
    hy = D.golden_hyper(g, case)
    return D.State(D.golden_init(g, case), hy, learner=hy["learner"], lr=hy["lr"])


def run_steps(g, case, **kw):
    """[(loss, {name: value})] after every step of the case"""
    R = D.golden_matrix(g, case)
    st = make_state(g, case)
    out = []
    for users, items, labels in D.golden_batches(g, case):
        loss = D.step(st, R, users, items, labels, **kw)
        out.append((loss, {k: v.copy() for k, v in st.var.items()}))
    return out, st


def first_miss(g, case, trace, tol=1e-9):
    """the first (step, name, error) beyond `tol` of the float64 trace, None when every loss and variable follows"""
    init = D.golden_init(g, case)
    for k, (loss, var) in enumerate(trace):
        want = float(g[case + "_loss_f64"][k])
        if not abs(loss - want) <= tol * max(1.0, abs(want)):
            return k, "loss", abs(loss - want)
        if case == "epoch" and k < len(trace) - 1:
            continue
        for name, v in var.items():
            err = np.abs(v - D.golden_var(g, case, init, name, 0 if case == "epoch" else k)).max()
            if not err <= tol:
                return k, name, err
    return None


def test_cases_are_the_fixture_s(golden):
    g = golden
    assert sorted(STEP_CASES) == sorted(str(c) for c in g["cases"])
    hy = {c: D.golden_hyper(g, c) for c in STEP_CASES + ("epoch",)}
    d = hy["default"]                                              # conf/DeepICF.properties
    assert (d["algorithm"], d["activation"], d["batch_norm"], d["layers"], d["d"], d["w"], d["regw"], d["beta"]) == \
        (1, -1, 1, [64, 32, 16], 16, 16, [10.0, 10.0], 0.5)
    p = hy["prod_nobn"]
    assert (p["algorithm"], p["activation"], p["batch_norm"], p["layers"], p["regw"], p["alpha"], p["beta"]) == \
        (0, 0, 0, [8], [], 0.5, 1.0)
    o = hy["odd"]
    assert (o["d"], o["w"], o["layers"], o["activation"], o["batch_norm"]) == (7, 5, [12, 5], 2, 1)
    assert len(o["regw"]) > len(o["layers"]) and 0.0 in o["regw"]
    assert hy["adagrad"]["learner"] == "adagrad" and hy["rmsprop"]["learner"] == "rmsprop"
    assert [len(b[0]) for b in D.golden_batches(g, "single")] == [1, 1, 1]
    sizes = g["epoch_sizes"]
    assert (sizes[:-1] == 16).all() and 0 < sizes[-1] < 16 and hy["epoch"]["lr"] == 0.001


def test_optimiser_forms_are_the_trace_s(golden):
    """what the stand-in's trace recorded: `bias` alone is applied by rows"""
    import json
    forms = json.loads(str(golden["forms_json"]))
    assert sorted(forms) == sorted(D.names(3, True))
    assert [k for k, f in forms.items() if f == "rows"] == ["bias"]


@pytest.mark.parametrize("case", STEP_CASES + ("epoch",))
def test_restatement_matches_the_f64_trace(golden, case):
    """every loss, and every variable (moving statistics included) after every step, within 1e-9 of the reference
    class's float64 run; the pre-norm biases under batch norm follow it too: the float64 run's rounding noise moves
    them by less than 1e-9, the restatement's exact zero by nothing"""
    trace, st = run_steps(golden, case)
    assert first_miss(golden, case, trace) is None
    if st.hyper["batch_norm"]:
        init = D.golden_init(golden, case)
        for i in range(len(st.hyper["layers"])):
            assert np.array_equal(st.var["b%d" % i], init["b%d" % i].astype(np.float64))


@pytest.mark.parametrize("case", ("default", "epoch"))
def test_predict_matches_the_f64_trace(golden, case):
    g = golden
    _, st = run_steps(g, case)
    got = D.predict(D.golden_matrix(g, case), st.var, st.hyper, g["predict_users"])
    before = {k: v.copy() for k, v in st.var.items()}
    assert np.abs(got - g["predict_%s_f64" % case]).max() <= 1e-9
    cand = np.take_along_axis(got, g["predict_cand"].astype(np.int64), axis=1)
    assert np.abs(cand - g["predict_%s_cand_f64" % case]).max() <= 1e-9
    assert all(np.array_equal(before[k], st.var[k]) for k in before)           # predict() moves nothing
    mv = st.var["mv0"]
    assert np.abs(mv - 1.0).max() > 0.1                            # the moving statistics are away from 0 / 1


VARIANTS = {                                  # mistake -> (how the restatement makes it, a case that must tell)
    "moving statistics used in training": (dict(variant="moving_in_training"), "default"),
    "Bessel's correction dropped": (dict(bessel=False), "default"),
    "the 1e-7 of the loss dropped": (dict(variant="no_eps"), "saturated"),
    "mean loss turned into a sum": (dict(variant="sum_loss"), "default"),
    "regw applied to every layer": (dict(variant="regw_all"), "default"),
    "the sum dy xhat term dropped": (dict(variant="no_xhat_term"), "default"),
    "the history mask": (dict(mask="history"), "default"),
    "embedding_Q applied by rows": (dict(variant="q_rows"), "adagrad"),
    "the exponent of num_idx negated": (dict(variant="neg_alpha"), "prod_nobn"),
}


@pytest.mark.parametrize("mistake", sorted(VARIANTS))
def test_the_trace_tells_each_mistake(golden, mistake):
    kw, case = VARIANTS[mistake]
    trace, _ = run_steps(golden, case, **kw)
    assert first_miss(golden, case, trace, tol=1e-7) is not None


def test_gradients_against_autograd(golden):
    """the hand-written gradients of case `odd` against torch autograd on the same float64 expression"""
    g, case = golden, "odd"
    hy = D.golden_hyper(g, case)
    R = D.golden_matrix(g, case)
    V = {k: np.asarray(v, np.float64) for k, v in D.golden_init(g, case).items()}
    users, items, labels = D.golden_batches(g, case)[0]
    loss, G, _, _ = D.loss_and_gradients(V, R, users, items, labels, hy)
    T = {k: torch.tensor(V[k], dtype=torch.float64, requires_grad=k in G) for k in V}
    inst = F.instances(R, users, items, labels, False)
    ids, m, item, n = D.padded(R, inst, "reference")
    ids, m, item, n = torch.from_numpy(ids), torch.from_numpy(m), torch.from_numpy(item), torch.from_numpy(n)
    table = torch.cat([T["c1"], torch.zeros(1, hy["d"], dtype=torch.float64)])
    c, q = table[ids], T["Q"][item]
    x = torch.cat([c, q[:, None, :].expand(-1, c.shape[1], -1)], dim=2) if hy["algorithm"] else c * q[:, None, :]
    a = torch.tanh(x @ T["W"] + T["b"])
    assert hy["activation"] == 2
    e = torch.exp(a @ T["h"]) * m
    p = ((e / e.sum(1, keepdim=True) ** hy["beta"])[:, :, None] * c).sum(1)
    x = (n ** hy["alpha"])[:, None] * p * q
    for i in range(len(hy["layers"])):
        z = x @ T["W%d" % i] + T["b%d" % i]
        mu, var = z.mean(0), z.var(0, unbiased=False)
        x = torch.relu(T["gamma%d" % i] * (z - mu) / torch.sqrt(var + D.BN_EPS) + T["beta%d" % i])
    prob = torch.sigmoid((x @ T["Wout"] + T["bout"]).sum(1) + T["bias"][item])
    y = torch.from_numpy(np.asarray(labels, np.float64))
    total = (-y * torch.log(prob + 1e-7) - (1 - y) * torch.log(1 - prob + 1e-7)).mean()
    total = total + hy["regs"][0] * 0.5 * (T["Q"] ** 2).sum() + hy["regs"][1] * 0.5 * (T["c1"] ** 2).sum() + \
        hy["regs"][2] * 0.5 * (T["W"] ** 2).sum()
    for i in range(min(len(hy["layers"]), len(hy["regw"]))):
        if hy["regw"][i] > 0:
            total = total + hy["regw"][i] * 0.5 * (T["W%d" % i] ** 2).sum()
    assert abs(float(total.detach()) - loss) <= 1e-12 * abs(loss)
    grads = torch.autograd.grad(total, [T[k] for k in G])
    for k, auto in zip(G, grads):
        scale = max(1.0, float(auto.abs().max()))
        if k.startswith("b") and k[1:].isdigit():                  # pre-norm: autograd leaves rounding noise, we zero
            assert float(auto.abs().max()) <= 1e-12 and not G[k].any()
        else:
            assert np.abs(G[k] - auto.numpy()).max() <= 1e-12 * scale, k


def test_steps_hold_the_edges(golden):
    """every 6-instance step: a repeated (user, item), a target that is in another instance's history, and a positive
    that pools nothing but the padding row"""
    g = golden
    for case in ("default", "prod_nobn", "odd", "adagrad", "rmsprop", "saturated"):
        R = D.golden_matrix(g, case)
        for users, items, labels in D.golden_batches(g, case):
            inst = F.instances(R, users, items, labels, False)
            assert len(inst) == 6
            pairs = [(u, i) for u, i, _, _, _ in inst]
            assert len(set(pairs)) < len(pairs)
            hists = [set(F.history(R, u, e).tolist()) for u, _, e, _, _ in inst]
            assert any(i in h for k, (_, i, _, _, _) in enumerate(inst) for j, h in enumerate(hists) if j != k)
            ids, m, _, n = D.padded(R, inst, "reference")
            empty = [k for k, h in enumerate(hists) if not h]
            assert empty and all(m[k].sum() == 1 and ids[k, 0] == R.shape[1] and n[k] == 1 for k in empty)


def test_the_defaults_row_equals_the_properties_file():
    """defaults.MODELS["DeepICF"] against the copy of the reference's conf/DeepICF.properties under tests/golden/"""
    import configparser
    import os
    from conftest import GOLDEN
    from neurec_amd import defaults
    ref = configparser.ConfigParser()
    ref.optionxform = str
    assert ref.read(os.path.join(GOLDEN, "neurec_conf", "conf", "DeepICF.properties"))
    want = dict(ref["hyperparameters"])
    assert dict(defaults.MODELS["DeepICF"]) == want and [k for k, _ in defaults.MODELS["DeepICF"]] == list(want)
    assert (want["layers"], want["regw"], want["algorithm"], want["batch_norm"], want["activation"]) == \
        ("[64,32,16]", "[10,10]", "1", "1", "Relu")
