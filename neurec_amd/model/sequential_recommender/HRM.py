"""HRM on the HIP engine.

Reference: Pengfei Wang et al., "Learning Hierarchical Representation Model for NextBasket Recommendation." SIGIR 2015.
Plugin-compatible with model/sequential_recommender/HRM.py: same constructor, config keys (conf/HRM.properties: epochs,
batch_size, embedding_size, reg_mf, learning_rate, learner, pre_agg, session_agg, high_order, num_neg, loss_function,
init_method, stddev, verbose), log lines and `predict` contract.  The per-batch `sess.run((loss, optimizer))` is
neurec_amd/hrm.py (csrc/hrm.hip); the instances come from the device stream of the time-order pointwise sampler at
high_order = L, its `recent` field as it comes (both aggregations are symmetric in their inputs).

Deviations, on purpose:
(a) A user without train items scores <P_u, V_i>: it is pooled over the user alone (the reference raises KeyError).
(b) At high_order = 1 the reference's predict() feeds [N, 1] recents into a graph built for [N] and its concat fails on
    rank; here the user is pooled with its last item, which is what training does.
Kept: predict() slices `seq[len(seq) - L:]`, so a user with 0 < |R_u| < L is pooled over its last min(L - |R_u|, |R_u|)
items (the mean over that many); pre_agg / session_agg values other than "max" mean avg.  Candidate mode returns the
candidates' entries of the full-mode rows.
"""
import numpy as np

from ...util import timer
from ...util.tool import get_initializer
from ..AbstractRecommender import SeqAbstractRecommender
from .._common import predict_scores, require_single_gpu, train_time_order_model

DEVIATIONS = "users without train items score <P_u, V_i> (the reference raises KeyError); at high_order = 1 " \
             "predict() pools the user with its last item as training does (the reference's concat fails on rank); " \
             "kept: users with fewer than high_order train items are pooled over their last min(L - |R_u|, |R_u|)"


def last_items_table(train_dict, num_users, high_order):
    """int32 [U, L]: the items predict() pools user u over — HRM.py:144,157 slices `seq[len(seq) - L:]`, which for
    0 < |R_u| < L has a NEGATIVE start and yields the last min(L - |R_u|, |R_u|) items (kept: 2 items at L = 3 give the
    last 1, 4 items at L = 6 the last 2); -1 fills the remaining columns and the rows of users without train items"""
    last = np.full((num_users, high_order), -1, dtype=np.int32)
    for user, items in train_dict.items():
        items = list(items)
        tail = items[len(items) - high_order:] if len(items) else []
        last[user, :len(tail)] = tail
    return last


class HRM(SeqAbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(HRM, self).__init__(dataset, conf)
        self.learning_rate = conf["learning_rate"]
        self.embedding_size = conf["embedding_size"]
        self.learner = conf["learner"]
        self.num_epochs = conf["epochs"]
        self.reg_mf = conf["reg_mf"]
        self.pre_agg = conf["pre_agg"]
        self.loss_function = conf["loss_function"]
        self.session_agg = conf["session_agg"]
        self.batch_size = conf["batch_size"]
        self.high_order = conf["high_order"]
        self.verbose = conf["verbose"]
        self.num_negatives = conf["num_neg"]
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.dataset = dataset
        self.train_dict = dataset.get_user_train_dict(by_time=True)       # HRM.py:36: csr_to_user_dict_bytime
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None
        self.last_items = None

    def build_graph(self):
        from ...hrm import HRMEngine
        require_single_gpu("HRM")
        init = get_initializer(self.init_method, self.stddev, seed=2017)   # main.py:12
        P = init([self.num_users, self.embedding_size])                    # creation order of HRM.py:49-52
        V = init([self.num_items, self.embedding_size])
        last = last_items_table(self.train_dict, self.num_users, self.high_order)
        self.engine = HRMEngine(P, V, self.learning_rate, self.reg_mf, self.batch_size, self.high_order,
                                pre_agg=self.pre_agg, session_agg=self.session_agg, loss=self.loss_function,
                                learner=self.learner, last_items=last)
        self.last_items = self.engine.last_items

    # ---------- training process -------
    def train_model(self):
        engine, L = self.engine, self.high_order
        train_time_order_model(self, L, False, DEVIATIONS,
                               step=lambda u, recent, i, y, out: engine.step(u, recent.reshape(-1, L), i, y, out))

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def get_eval_factors(self):
        """Device tables for the evaluator's on-GPU factor path: h_u against V."""
        return self.engine.eval_factors()

    def predict(self, user_ids, candidate_items_userids=None):
        P, Q = self.engine.eval_factors()
        return predict_scores(P, Q, user_ids, candidate_items_userids)
