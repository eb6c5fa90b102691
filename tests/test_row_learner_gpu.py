"""neurec_amd/row_learner.py on the device: RowLearner hands E.optimizer_rows / E.adam_sparse / E.adam_dense /
DenseLearner the constants util/learner.py means — two steps on a [5, 3] table and on a 1-D [5] table (taken as [5, 1])
bit-equal to tests/primitives_restatement.py fed those constants, the comparison test_primitives_gpu.py makes for the
kernels themselves."""
import numpy as np
import pytest

import primitives_restatement as R

pytestmark = pytest.mark.gpu

LR, MOMENTUM = 0.05, 0.75                        # a momentum that is not the default: it must reach both kernels
KINDS = ("gd", "adagrad", "rmsprop", "momentum")
SHAPES = ((5, 3), (5,))


def _hyper(kind):
    """(hyper1, hyper2, eps) of learner.py:2-14: tf.train.RMSPropOptimizer(lr) is decay 0.9, momentum 0, epsilon 1e-10"""
    return {"rmsprop": (0.9, 0.0, 1e-10), "momentum": (MOMENTUM, 0.0, 0.0)}.get(kind, (0.0, 0.0, 0.0))


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _bits(got, want, what):
    assert (got is None) == (want is None), what
    if want is not None:
        assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (what, got, want)


def _learner(kind):
    from neurec_amd import engine as E
    from neurec_amd.row_learner import RowLearner
    return RowLearner(kind, LR, MOMENTUM, E.AdamState(LR))


def _host_slots(kind, shape):
    from neurec_amd.row_learner import slot_init
    first, two = slot_init(kind)
    return (None if first is None else np.full(shape, first, np.float32),
            np.zeros(shape, np.float32) if two else None)


@pytest.mark.parametrize("shape", SHAPES, ids=("5x3", "5"))
@pytest.mark.parametrize("kind", KINDS)
def test_apply_bit_equal_to_the_restated_rows(kind, shape):
    """slots() at TF's initial values, flag() five zero bytes; after each of two steps var and the slots bit-equal to
    primitives_restatement.optimizer_rows, unflagged gradient rows untouched, flagged ones and every flag zero"""
    import torch
    rl = _learner(kind)
    rs = np.random.RandomState(3)
    var = rs.randn(*shape).astype(np.float32)
    s0, s1 = _host_slots(kind, shape)
    dvar = _dev(var)
    ds0, ds1 = rl.slots(dvar)
    _bits(_np(ds0), s0, (kind, "initial slot0"))
    _bits(_np(ds1), s1, (kind, "initial slot1"))
    dflag = rl.flag(5, dvar.device)
    assert dflag.dtype == torch.uint8 and dflag.is_cuda and _np(dflag).tolist() == [0] * 5
    rows = lambda a: None if a is None else a.reshape(5, -1)          # views: the restatement works in place
    seen = np.zeros(5, np.uint8)
    for step in range(2):
        flag = R.flag_pattern("some", 5, rs)
        seen |= flag
        g = (0.1 * rs.randn(*shape)).astype(np.float32)
        dg = _dev(g)
        dflag.copy_(_dev(flag))
        before, still = var.copy(), np.flatnonzero(flag == 0)
        rl.apply(dvar, ds0, ds1, dg, dflag)
        R.optimizer_rows(kind, rows(var), rows(s0), rows(s1), rows(g), flag, LR, *_hyper(kind))
        for name, dev, want in (("var", dvar, var), ("slot0", ds0, s0), ("slot1", ds1, s1), ("grad", dg, g)):
            _bits(_np(dev), want, (kind, shape, step, name))
        _bits(_np(dvar)[still], before[still], (kind, shape, step, "unflagged rows"))
        assert not _np(dflag).any() and not flag.any()
    assert 0 < seen.sum() < 5                    # the pattern flagged some rows and left some alone


def test_adam_is_the_sparse_sweep():
    """flag() is None; apply() on copies byte-equal to E.adam_sparse called directly, over two steps of one AdamState"""
    from neurec_amd import engine as E
    rl = _learner("adam")
    assert rl.flag(5, "cuda") is None
    rs = np.random.RandomState(4)
    for shape in SHAPES:
        var = rs.randn(*shape).astype(np.float32)
        a, b = _dev(var), _dev(var)
        (am, av), (bm, bv) = rl.slots(a), rl.slots(b)
        assert not _np(am).any() and not _np(av).any() and am.shape == a.shape and av.shape == a.shape
        for step in range(2):
            g = (0.1 * rs.randn(*shape)).astype(np.float32)
            ga, gb = _dev(g), _dev(g)
            rl.apply(a, am, av, ga, None)
            E.adam_sparse(b, bm, bv, gb, rl.adam)
            for name, x, y in (("var", a, b), ("m", am, bm), ("v", av, bv), ("grad", ga, gb)):
                _bits(_np(x), _np(y), (shape, step, name))
            assert not np.array_equal(_np(a), var)
            rl.adam.advance()


@pytest.mark.parametrize("clear", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_apply_dense_bit_equal_to_the_restated_dense(kind, clear):
    """two tensors ([7] and [3, 4]) in one call, two steps: var and slots bit-equal to
    primitives_restatement.optimizer_dense; the gradient is zero afterwards (clear_grad=True) or untouched"""
    rl = _learner(kind)
    rs = np.random.RandomState(5)
    host, dev = [], []
    for shape in ((7,), (3, 4)):
        var = rs.randn(*shape).astype(np.float32)
        host.append([var] + list(_host_slots(kind, shape)))
        dvar = _dev(var)
        dev.append((dvar,) + rl.slots(dvar))
    for step in range(2):
        gs = [(0.1 * rs.randn(*h[0].shape)).astype(np.float32) for h in host]
        dgs = [_dev(g) for g in gs]
        rl.apply_dense([d + (dg,) for d, dg in zip(dev, dgs)], clear_grad=clear)
        for (var, s0, s1), (dvar, ds0, ds1), g, dg in zip(host, dev, gs, dgs):
            R.optimizer_dense(kind, var, s0, s1, g, LR, *_hyper(kind), clear_grad=clear)
            for name, d, want in (("var", dvar, var), ("slot0", ds0, s0), ("slot1", ds1, s1), ("grad", dg, g)):
                _bits(_np(d), want, (kind, clear, step, name))
            assert g.any() != clear


@pytest.mark.parametrize("clear", (False, True))
def test_apply_dense_adam_is_apply_adam(clear):
    """byte-equal to E.adam_dense called directly on copies, the gradient cleared or not as asked"""
    from neurec_amd import engine as E
    rl = _learner("adam")
    rs = np.random.RandomState(6)
    var, g = rs.randn(3, 4).astype(np.float32), (0.1 * rs.randn(3, 4)).astype(np.float32)
    a, b, ga, gb = _dev(var), _dev(var), _dev(g), _dev(g)
    (am, av), (bm, bv) = rl.slots(a), rl.slots(b)
    rl.apply_dense([(a, am, av, ga)], clear_grad=clear)
    E.adam_dense(b, bm, bv, gb, rl.adam, clear_grad=clear)
    for name, x, y in (("var", a, b), ("m", am, bm), ("v", av, bv), ("grad", ga, gb)):
        _bits(_np(x), _np(y), (clear, name))
    assert _np(ga).any() != clear and not np.array_equal(_np(a), var)
