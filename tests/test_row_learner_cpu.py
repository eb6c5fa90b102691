"""neurec_amd/row_learner.py and the table helpers of neurec_amd/model/_common.py on the host: the one copy of the
slots' initial values, the refusals of learner.py as every engine raises them, and the last-item tables on hand-written
sequences (a user without items, with fewer than L, exactly L and more than L; user 5 is absent from the dict)."""
import numpy as np
import pytest

SEQS = {0: [], 1: [4], 2: [3, 9], 3: [5, 1, 7], 4: [2, 8, 6, 0, 3]}


def test_slot_init_of_the_five_learners():
    """learner.py:2-14 as TF-1.12 creates the slots: adam m = v = 0; gd none; adagrad's accumulator 1e-8; rmsprop's rms
    ones and its momentum zeros; momentum's accumulator zeros"""
    from neurec_amd.row_learner import slot_init
    assert slot_init("adam") == (0.0, True)
    assert slot_init("gd") == (None, False)
    assert slot_init("adagrad") == (1e-8, False)
    assert slot_init("rmsprop") == (1.0, True)
    assert slot_init("momentum") == (0.0, False)
    with pytest.raises(KeyError):
        slot_init("sgd")


def test_check_loss_learner_accepts_and_refuses_as_the_engines():
    from neurec_amd import engine as E
    from neurec_amd.row_learner import check_loss_learner
    learners = ("adam", "gd", "adagrad", "rmsprop", "momentum")
    for pairwise, table in ((True, E.PAIRWISE_LOSSES), (False, E.POINTWISE_LOSSES)):
        for loss, code in table.items():
            for learner in learners:
                assert check_loss_learner(loss, learner, pairwise) == (loss, learner, code)
                assert check_loss_learner(loss.upper(), learner.capitalize(), pairwise) == (loss, learner, code)
    assert sorted(E.PAIRWISE_LOSSES) == ["bpr", "hinge", "square"]
    assert sorted(E.POINTWISE_LOSSES) == ["cross_entropy", "square"]
    for loss, pairwise in (("cross_entropy", True), ("bpr", False), ("hinge", False), ("log", True), ("", False)):
        with pytest.raises(Exception, match="^please choose a suitable loss function$") as e:
            check_loss_learner(loss, "adam", pairwise)
        assert type(e.value) is Exception
    for learner in ("sgd", "adadelta", ""):
        with pytest.raises(ValueError, match="^please select a suitable optimizer$"):
            check_loss_learner("square", learner, True)
    with pytest.raises(Exception, match="loss function"):            # the loss is looked at first
        check_loss_learner("log", "sgd", False)


def test_last_item_of():
    from neurec_amd.model._common import last_item_of
    last = last_item_of(SEQS, 6)
    assert last.dtype == np.int32 and last.tolist() == [-1, 4, 9, 7, 3, -1]


def test_last_items_table_equals_the_two_functions_it_replaces():
    """the expected arrays are what model/sequential_recommender/Fossil.py's and neurec_amd/fpmcplus.py's
    last_items_table both returned on SEQS before they became this one function"""
    from neurec_amd.fpmcplus import last_items_table as from_engine_module
    from neurec_amd.model._common import last_items_table
    from neurec_amd.model.sequential_recommender.Fossil import last_items_table as from_fossil
    assert from_engine_module is last_items_table and from_fossil is last_items_table
    want = {3: [[-1, -1, -1], [4, -1, -1], [3, 9, -1], [5, 1, 7], [6, 0, 3], [-1, -1, -1]],
            2: [[-1, -1], [4, -1], [3, 9], [1, 7], [0, 3], [-1, -1]],
            1: [[-1], [4], [9], [7], [3], [-1]]}
    for L, rows in want.items():
        got = last_items_table(SEQS, 6, L)
        assert got.dtype == np.int32 and got.shape == (6, L) and got.tolist() == rows, L
        arrays = {u: np.asarray(s, np.int64) for u, s in SEQS.items()}
        assert np.array_equal(last_items_table(arrays, 6, L), got)


def test_hrm_keeps_its_own_sliced_table():
    """HRM's (and NPE's) table keeps the reference's negative-start slice and is a different function: 2 items at
    L = 3 give the last 1"""
    from neurec_amd.model._common import last_items_table
    from neurec_amd.model.sequential_recommender import HRM, NPE
    assert NPE.last_items_table is HRM.last_items_table and HRM.last_items_table is not last_items_table
    assert HRM.last_items_table(SEQS, 6, 3).tolist() == \
        [[-1, -1, -1], [4, -1, -1], [9, -1, -1], [5, 1, 7], [6, 0, 3], [-1, -1, -1]]
