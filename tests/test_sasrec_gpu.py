"""SASRec on the GPU (csrc/sasrec.hip through neurec_amd/sasrec.py): every step of the reference class's trace, the
recorded epoch through run_schedule, the users' embeddings and predict(), the edge shapes of the step on its gradients,
awkward logits, masks that drop whole rows, determinism, empty work, ids outside the table, the refusals and the
drop-in run through neurec_amd.main."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import sasrec_restatement as P
from sasrec_restatement import CASES
from test_sasrec_cpu import awkward_batch, case_inputs, golden_table
from test_gru4rec_gpu import _close, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("tfgraph_sasrec")


def _engine(T, nb, h, max_batch, lr=0.001, l2=0.0, rate=0.0, seed=2017):
    from neurec_amd.sasrec import BLOCK_VARS, SASRecEngine
    blocks = [[T["b%d_%s" % (i, n)] for n in BLOCK_VARS] for i in range(nb)]
    return SASRecEngine(T["item_emb"], T["pos_emb"], blocks, (T["lnf_beta"], T["lnf_gamma"]), lr, l2, max_batch, h, rate,
                        seed=seed)


def _dev(eng, a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(eng.item_emb.device)


def _masks(eng, masks):
    return None if masks is None else [_dev(eng, m, np.uint8) for m in masks]


def _tables(eng):
    return {k: t.cpu().numpy() for k, t in eng.tables().items()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_match_the_reference_trace(golden, case):
    """Every variable after every step, and each step's loss, against the f64 trace: within 4x the reference's own
    f32-to-f64 distance of that step and tensor (read from the golden) plus 1e-5 max|want|.  Rows of item_emb outside
    <case>_rows_item_emb are bit-equal to their initial value; the gradient buffers are zero again afterwards."""
    import torch
    g = golden
    d, h, nb, L, l2, rate = CASES[case]
    names, init, feeds, masks = case_inputs(g, case)
    eng = _engine(init, nb, h, int(g["batch_step"]), float(g["lr"]), l2, rate)
    assert list(eng.tables()) == names
    loss2 = torch.zeros(2, device=eng.item_emb.device)
    for s, (seq, pos, neg) in enumerate(feeds):
        eng.step(seq, pos, neg, loss2, _masks(eng, None if masks is None else masks[s]))
        l64, l32 = float(g[case + "_loss_f64"][s]), float(g[case + "_loss_f32"][s])
        _close(np.asarray([loss2.sum().item()]), np.asarray([l64]), abs(l32 - l64), "%s step %d loss" % (case, s + 1))
        for name, got in _tables(eng).items():
            w64, w32 = (golden_table(g, case, tag, name, s) for tag in ("f64", "f32"))
            _close(got, w64, np.abs(w32 - w64).max(), "%s step %d %s" % (case, s + 1, name))
        still = np.setdiff1d(np.arange(len(init["item_emb"])), g[case + "_rows_item_emb"])
        assert bool(len(still)) == (l2 == 0)                      # the regulariser moves every row
        assert np.array_equal(eng.item_emb.cpu().numpy()[still], init["item_emb"][still]), (case, s)
    assert eng.t == len(feeds) and eng.skipped_steps == 0
    for name, G in eng.G.items():
        assert not G.any().item(), name


def test_the_recorded_epoch_ends_at_the_reference_tables(golden):
    """train_model()'s epoch of the golden (rate 0) through run_schedule, the last batch filled up with all-padded
    rows; the end tables under the trace's rule"""
    import torch
    g = golden
    d, h, nb, L, l2, _ = CASES["first"]
    names = P.table_names(nb)
    eng = _engine({k: g["epoch_init_" + k] for k in names}, nb, h, int(g["batch_epoch"]), float(g["lr"]), l2, 0.0)
    S = len(g["epoch_seq"])
    losses = torch.zeros((S, 2), device=eng.item_emb.device)
    eng.run_schedule(g["epoch_seq"], g["epoch_pos"], g["epoch_neg"], losses)
    assert eng.t == S and eng.skipped_steps == 0 and np.isfinite(losses.cpu().numpy()).all()
    for name, got in _tables(eng).items():
        w64, w32 = (golden_table(g, "epoch", tag, name, 0) for tag in ("f64", "f32"))
        _close(got, w64, np.abs(w32 - w64).max(), "epoch end %s" % name)


def test_user_embeddings_and_predict_match_the_reference(golden):
    """seq[:, -1, :] and predict(), full and candidate mode, after the trained case, under the trace's rule; a user
    without train items scores the all-padded row"""
    import torch
    g = golden
    case = P.PREDICT_CASE
    d, h, nb, L, l2, rate = CASES[case]
    names, init, feeds, masks = case_inputs(g, case)
    eng = _engine(init, nb, h, int(g["batch_step"]), float(g["lr"]), l2, rate)
    loss2 = torch.zeros(2, device=eng.item_emb.device)
    for s, (seq, pos, neg) in enumerate(feeds):
        eng.step(seq, pos, neg, loss2, _masks(eng, masks[s]))
    eng.set_sequences(g["seq_ptr"], g["seq"])
    users, cand = g["predict_users"], g["predict_cand"]
    H = eng.user_embeddings(users).cpu().numpy()
    _close(H, g["user_emb_f64"], np.abs(g["user_emb_f32"] - g["user_emb_f64"]).max(), "user embeddings")
    got = eng.score(users)
    assert got.is_cuda and tuple(got.shape) == (len(users), eng.n_items)
    got = got.cpu().numpy()
    _close(got, g["predict_f64"], np.abs(g["predict_f32"] - g["predict_f64"]).max(), "predict")
    got_c = np.stack([got[k][c] for k, c in enumerate(cand)])
    _close(got_c, g["predict_cand_f64"], np.abs(g["predict_cand_f32"] - g["predict_cand_f64"]).max(),
           "predict, candidates")
    empty = np.flatnonzero(np.diff(g["seq_ptr"]) == 0)
    who = [int(empty[0])] if len(empty) else [len(g["seq_ptr"]) + 5]           # or a user outside the data
    T = _tables(eng)
    row = eng.score(who).cpu().numpy()[0]
    want = T["lnf_beta"].astype(np.float64) @ (T["item_emb"].astype(np.float64) * np.sqrt(d)).T
    assert np.abs(row - want).max() <= 1e-5 * np.abs(want).max()


# ------------------------------------------------------------------ edges of the step
def _batch(I, L, B, seed, lens=None):
    rs = np.random.RandomState(seed)
    seq, pos, neg = (np.full((B, L), I, np.int32) for _ in range(3))
    lens = rs.randint(1, L + 1, B).tolist() if lens is None else lens
    for b in range(B):
        n = min(lens[b], L)
        if n:
            seq[b, L - n:], pos[b, L - n:], neg[b, L - n:] = (rs.randint(0, I, n) for _ in range(3))
    return seq, pos, neg


def _check_gradients(T, seq, pos, neg, I, h, rate=0.0, l2=0.0, masks=None, tol=1e-5, floor=0.0):
    """gradients() against the float64 restatement in the reference's full-mask form: 1e-5 max|want| per tensor (fp32
    sums of at most a few hundred terms of the tensor's own size, each carrying a few 2^-24).  Adam is left out on
    purpose: its first step is lr sign(g) and hides the size of an error.  Where a gradient is zero in exact arithmetic
    (bk: a softmax ignores a shift) `floor` bounds the noise instead: callers pass 1e-6 of the largest gradient."""
    import torch
    nb = (len(T) - 4) // 14
    B = len(seq)
    eng = _engine(T, nb, h, B, 0.001, l2, rate)
    before = _tables(eng)
    loss2 = torch.zeros(2, device=eng.item_emb.device)
    eng.gradients(seq, pos, neg, loss2, _masks(eng, masks))
    want_loss, G = P.gradients(T, seq, pos, neg, I, h, rate, l2, masks, "mask")
    got_loss = float(loss2.cpu().numpy().astype(np.float64).sum())
    print("loss: got %.9g want %.9g" % (got_loss, want_loss))
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss)
    biggest = max(np.abs(v).max() for v in G.values())
    for name, want in G.items():
        got = eng.G[name].cpu().numpy()
        err = np.abs(got - want).max()
        print("%s: err %.3g, max|want| %.3g" % (name, err, np.abs(want).max()))
        assert np.isfinite(got).all() and err <= tol * np.abs(want).max() + floor * biggest, (name, err)
    for name, t in _tables(eng).items():                           # gradients() moves no table
        assert np.array_equal(t, before[name]), name
    return eng


@pytest.mark.parametrize("d,h,nb,L,B", [
    (6, 2, 1, 5, 1),              # B = 1
    (6, 3, 2, 1, 5),              # L = 1
    (1, 1, 1, 4, 3),              # d = 1: every normalised row is beta
    (128, 128, 1, 6, 3),          # 128 heads of width 1
    (128, 1, 1, 6, 3),            # one head of width 128 (both column halves of a wavefront)
    (8, 2, 1, 200, 2),            # the longest sequence
    (10, 2, 4, 7, 4),             # 4 blocks
    (65, 5, 2, 9, 70),            # a width just past a wavefront, more rows than one chunk of the weight gradients
])
def test_gradients_at_the_edge_shapes(d, h, nb, L, B):
    I = 23
    T = P.init_tables(I, d, L, nb, seed=d + L)
    seq, pos, neg = _batch(I, L, B, seed=B)
    _check_gradients(T, seq, pos, neg, I, h, l2=0.01, floor=1e-6)


def test_the_epsilon_sits_inside_the_root():
    """embeddings of 1e-4: the first layer norm's variance is about its epsilon, 1e-8, so sqrt(var + eps) and
    sqrt(var) + eps differ by tens of per cent"""
    I, d, h, nb, L, B = 9, 6, 2, 1, 4, 3
    T = P.init_tables(I, d, L, nb, seed=12)
    T["item_emb"], T["pos_emb"] = (T["item_emb"] * 3e-5).astype(np.float32), (T["pos_emb"] * 3e-4).astype(np.float32)
    seq, pos, neg = _batch(I, L, B, seed=3)
    x = T["item_emb"][seq[seq != I]] * np.sqrt(d)
    assert 1e-10 < x.var(-1).max() < 1e-7
    _check_gradients(T, seq, pos, neg, I, h, floor=1e-6)


def test_gradients_of_a_mixed_batch_with_given_masks():
    """empty, one-item, full and truncated-to-full rows, a repeated item in one row, the same item as positive and
    negative, and masks that drop a whole row: a real position zeroed at the embedding is a masked key, and the one-item
    row's only query then sees no key at all — the uniform softmax over its L - 1 padded keys and itself"""
    I, d, h, nb, L, B = 9, 6, 2, 2, 5, 7
    T, seq, pos, neg, masks = awkward_batch(I, L, d, h, nb, B, 5)
    eng = _check_gradients(T, seq, pos, neg, I, h, rate=0.4, l2=0.01, masks=masks, floor=1e-6)
    assert eng.G["b0_bv"].abs().max().item() > 0


def test_the_repeated_item_sums_its_slots():
    """an item that is a row's input twice, another row's positive and a third row's negative: its gradient row is the
    sum of the four slots"""
    I, d, h, L = 9, 4, 1, 3
    T = P.init_tables(I, d, L, 1, seed=3)
    seq = np.asarray([[5, 5, 1], [I, 2, 3], [I, I, 4]], np.int32)
    pos = np.asarray([[5, 1, 5], [I, 3, 5], [I, I, 6]], np.int32)
    neg = np.asarray([[7, 7, 5], [I, 8, 0], [I, I, 5]], np.int32)
    eng = _check_gradients(T, seq, pos, neg, I, h, floor=1e-6)
    G = eng.G["item_emb"].cpu().numpy()
    assert np.abs(G[5]).max() > 0


def test_awkward_logits():
    """saturated positives and negatives: sigmoid(p) is 0 and 1 - sigmoid(n) is 0 in float32, the 1e-24 terms decide the
    loss (-log(1e-24) each) and the gradient is exactly zero there, as the reference's expressions give it — a softplus
    would give |logit| and a gradient of 1.  The float64 restatement is asked for the float32 behaviour: run in float32."""
    import torch
    I, d, h, nb, L, B = 11, 8, 1, 1, 4, 3
    T = P.init_tables(I, d, L, nb, seed=8)
    T["item_emb"] = (T["item_emb"] * 40).astype(np.float32)
    seq, pos, neg = _batch(I, L, B, seed=2, lens=[4, 2, 3])
    eng = _engine(T, nb, h, B)
    loss2 = torch.zeros(2, device=eng.item_emb.device)
    eng.gradients(seq, pos, neg, loss2)
    want_loss, G = P.gradients(T, seq, pos, neg, I, h, 0.0, 0.0, None, "mask", np.float32)
    got = float(loss2[0].item())
    print("loss got %.7g want %.7g" % (got, want_loss))
    cap = -np.log(np.float32(1e-24))
    assert want_loss > cap / 4                                       # some term sits at the cap
    assert np.isfinite(got) and abs(got - want_loss) <= 1e-4 * abs(want_loss)
    for name, want in G.items():
        g = eng.G[name].cpu().numpy()
        assert np.isfinite(g).all(), name
    # every target saturated on both sides: the loss is exactly 2 * -log(1e-24), every gradient exactly zero
    T2 = dict(T)
    T2["item_emb"] = np.zeros_like(T["item_emb"])
    T2["item_emb"][1], T2["item_emb"][2] = -50.0, 50.0
    T2["lnf_beta"], T2["lnf_gamma"] = np.ones(d, np.float32), np.zeros(d, np.float32)
    seq2 = np.asarray([[I, 3, 4, 5]], np.int32)
    pos2 = np.asarray([[I, 1, 1, 1]], np.int32)
    neg2 = np.asarray([[I, 2, 2, 2]], np.int32)
    eng2 = _engine(T2, nb, h, 1)
    eng2.gradients(seq2, pos2, neg2, loss2)
    assert abs(float(loss2[0].item()) - 2 * cap) <= 1e-5 * 2 * cap
    for name, G2 in eng2.G.items():
        assert not G2.any().item(), name


def test_two_runs_are_bit_identical_and_the_buffers_end_zero():
    import torch
    I, d, h, nb, L, B = 40, 50, 1, 2, 12, 33
    T = P.init_tables(I, d, L, nb, seed=4)
    seq, pos, neg = _batch(I, L, B, seed=9)
    runs = []
    for _ in range(2):
        eng = _engine(T, nb, h, B, rate=0.5, l2=0.01, seed=77)
        loss2 = torch.zeros(2, device=eng.item_emb.device)
        eng.gradients(seq, pos, neg, loss2)
        grads = {k: v.cpu().numpy().copy() for k, v in eng.G.items()}
        eng.apply()
        for name, G in eng.G.items():
            assert not G.any().item(), name
        eng.step(seq, pos, neg, loss2)                              # the generator's second step differs from its first
        runs.append((grads, _tables(eng), loss2.cpu().numpy().copy()))
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k
    assert np.array_equal(runs[0][2], runs[1][2])
    # the generator keeps about 1 - rate of a site and the scale 1 / (1 - rate) is there: with rate 0.5 the gradients
    # differ from the rate-0 ones, and an all-ones given mask at rate 0.5 doubles x at the embedding
    eng0 = _engine(T, nb, h, B, rate=0.0)
    eng0.gradients(seq, pos, neg, loss2)
    assert not np.array_equal(eng0.G["b0_Wq"].cpu().numpy(), runs[0][0]["b0_Wq"])


def test_the_scale_of_a_given_mask():
    """1 / (1 - rate): all-ones masks at rate 0.5 against the restatement"""
    I, d, h, nb, L, B = 9, 6, 2, 1, 4, 3
    T = P.init_tables(I, d, L, nb, seed=6)
    seq, pos, neg = _batch(I, L, B, seed=1)
    masks = [np.ones(s, np.uint8) for s in P.site_shapes(B, L, d, h, nb)]
    _check_gradients(T, seq, pos, neg, I, h, rate=0.5, masks=masks, floor=1e-6)


def test_empty_work_and_batches_without_a_target():
    import torch
    I, d, h, nb, L = 9, 6, 2, 1, 4
    T = P.init_tables(I, d, L, nb, seed=6)
    eng = _engine(T, nb, h, 4)
    before = _tables(eng)
    loss2 = torch.ones(2, device=eng.item_emb.device)
    none = np.zeros((0, L), np.int32)
    eng.step(none, none, none, loss2)                               # an empty batch
    assert eng.t == 0 and eng.skipped_steps == 0 and not loss2.any().item()
    pad = np.full((3, L), I, np.int32)
    loss2.fill_(1.0)
    eng.step(pad, pad, pad, loss2)                                  # every row empty: nothing launched, skipped
    assert eng.t == 0 and eng.skipped_steps == 1 and not loss2.any().item()
    seq, pos, neg = _batch(I, L, 3, seed=1)
    eng.step(_dev(eng, seq, np.int32), _dev(eng, pad, np.int32), _dev(eng, pad, np.int32), loss2)   # real rows, no target
    assert eng.t == 0 and eng.skipped_steps == 2 and np.isfinite(loss2.cpu().numpy()).all()
    for name, t in _tables(eng).items():
        assert np.array_equal(t, before[name]), name
    for name, G in eng.G.items():
        assert not G.any().item(), name
    losses = torch.zeros((2, 2), device=eng.item_emb.device)
    eng.run_schedule(np.stack([seq, seq]), np.stack([pad, pos]), np.stack([pad, neg]), losses)
    assert eng.t == 1 and eng.skipped_steps == 3
    eng.set_sequences(np.zeros(3, np.int64), np.zeros(0, np.int32))
    assert tuple(eng.score([]).shape) == (0, I) and tuple(eng.user_embeddings([]).shape) == (0, d)


def test_ids_outside_the_table():
    import torch
    I, d, h, nb, L = 9, 6, 2, 1, 4
    T = P.init_tables(I, d, L, nb, seed=6)
    eng = _engine(T, nb, h, 4)
    loss2 = torch.zeros(2, device=eng.item_emb.device)
    seq, pos, neg = _batch(I, L, 3, seed=1)
    for k, name in enumerate(("seq", "pos", "neg")):
        for bad in (-1, I + 1):
            arrs = [seq.copy(), pos.copy(), neg.copy()]
            arrs[k][1, -1] = bad
            with pytest.raises(ValueError, match=r"%s holds an item outside \[0, 9\]" % name):
                eng.step(arrs[0], arrs[1], arrs[2], loss2)
            with pytest.raises(ValueError, match=r"%s holds an item outside \[0, 9\]" % name):
                eng.run_schedule(arrs[0][None], arrs[1][None], arrs[2][None], loss2[None])
    with pytest.raises(ValueError, match=r"seq holds an item outside \[0, 9\)"):
        eng.set_sequences(np.asarray([0, 2]), np.asarray([1, 9]))
    assert eng.t == 0
    # device tensors are not read back: an id outside the table reads the zero row and its gradient is dropped
    bad = seq.copy()
    bad[1, -1] = I + 3
    eng.gradients(_dev(eng, bad, np.int32), _dev(eng, pos, np.int32), _dev(eng, neg, np.int32), loss2)
    as_pad = seq.copy()
    as_pad[1, -1] = I
    got = {k: v.cpu().numpy().copy() for k, v in eng.G.items()}
    for G in eng.G.values():
        G.zero_()
    eng.gradients(as_pad, pos, neg, loss2)
    for k, v in eng.G.items():
        assert np.array_equal(v.cpu().numpy(), got[k]), k


def test_refusals_on_the_device():
    import torch
    I, d, h, nb, L = 9, 6, 2, 1, 4
    T = P.init_tables(I, d, L, nb, seed=6)
    eng = _engine(T, nb, h, 2, rate=0.5)
    loss2 = torch.zeros(2, device=eng.item_emb.device)
    seq, pos, neg = _batch(I, L, 3, seed=1)
    with pytest.raises(ValueError, match="batch larger than max_batch"):
        eng.gradients(seq, pos, neg, loss2)
    with pytest.raises(ValueError, match=r"must be \[batch, max_len\]"):
        eng.gradients(seq[:2, :3], pos[:2, :3], neg[:2, :3], loss2)
    with pytest.raises(ValueError, match="masks: 1 sites, want 4"):
        eng.gradients(seq[:2], pos[:2], neg[:2], loss2, [_dev(eng, np.ones((2, L, d)), np.uint8)])
    with pytest.raises(ValueError, match=r"masks\[1\] must be"):
        eng.gradients(seq[:2], pos[:2], neg[:2], loss2,
                      [_dev(eng, np.ones(s), np.uint8) for s in ((2, L, d), (2, L, L), (2, L, d), (2, L, d))])
    with pytest.raises(ValueError, match="set_sequences"):
        eng.score([0])


# ------------------------------------------------------------------ the drop-in run
def test_sasrec_config_drops_in(tmp_path):
    """NeuRec.properties + conf/SASRec.properties (the reference's values) on ml-100k with by_time=True: two epochs
    through neurec_amd.main; the metrics header, the deviation line and two `epoch` lines, in order; predict()'s modes"""
    from neurec_amd.model.sequential_recommender.SASRec import DEVIATIONS
    model = _run(tmp_path, ["--recommender=SASRec", "--epochs=2"])
    eng = model.engine
    assert (eng.d, eng.L, eng.n_blocks, eng.n_heads, eng.max_batch, eng.rate) == (50, 50, 2, 1, 128, 0.5)
    assert eng.t == 2 * -(-len(model.user_pos_train) // 128) and eng.skipped_steps == 0
    folder = os.path.join(str(tmp_path), "log", "ml-100k", "SASRec")
    files = os.listdir(folder)
    assert len(files) == 1
    with open(os.path.join(folder, files[0])) as f:
        text = f.read()
    assert "SASRec's hyperparameters:" in text
    lines = [ln for ln in text.splitlines() if re.search(r"metrics:\t|epoch \d+:\t", ln) or DEVIATIONS in ln]
    kinds = ["m" if "metrics:" in ln else "d" if DEVIATIONS in ln else "e%s" % re.search(r"epoch (\d+):", ln).group(1)
             for ln in lines]
    assert kinds == ["m", "d", "e0", "e1"], kinds
    shown = np.asarray([float(x) for x in re.findall(r"epoch 1:\t(.+)", text)[0].split()])
    assert np.all(np.isfinite(shown)) and shown.max() > 0
    full = model.predict([0, 5, 9], None)
    assert tuple(full.shape) == (3, model.items_num) and full.is_cuda
    full = full.cpu().numpy()
    assert np.isfinite(full).all()
    cand = model.predict([0, 5], [[1, 2, 3], [7]])
    assert [len(c) for c in cand] == [3, 1] and np.array_equal(cand[0], full[0][[1, 2, 3]])
    assert np.array_equal(cand[1], full[1][[7]])


def test_plugin_refusals(tmp_path):
    with pytest.raises(ValueError, match="num_heads=3 does not divide hidden_units=50"):
        _run(tmp_path, ["--recommender=SASRec", "--epochs=1", "--num_heads=3"])
    with pytest.raises(NotImplementedError, match=r"max_len=201 is not supported \(1 to 200\)"):
        _run(tmp_path, ["--recommender=SASRec", "--epochs=1", "--max_len=201"])
