"""TransRec on the HIP engine.

Reference: Ruining He et al., "Translation-based Recommendation." in RecSys 2017.
Plugin-compatible with model/sequential_recommender/TransRec.py: same constructor, config keys
(conf/TransRec.properties: epochs, batch_size, embedding_size, reg_mf, learning_rate, learner, is_pairwise, num_neg,
loss_function, init_method, stddev, verbose), log lines and `predict` contract.  The per-batch
`sess.run((loss, optimizer))` is neurec_amd/transrec.py (csrc/transrec.hip); the instances come from the device streams
of the time-order samplers at high_order = 1.

Kept, as the class has them: training scores with the squared distance and predict() with the distance itself; the
`[iter ...]` line is commented out in the reference (TransRec.py:143-144) and is not logged here either.

Deviation, on purpose: a user without train items scores b_j - |P_u + T - Q_j| (the reference raises KeyError).
Candidate mode returns the candidates' entries of the full-mode rows.
"""
import numpy as np

from ...util import timer
from ...util.tool import get_initializer
from .._common import last_item_of, require_single_gpu, train_time_order_model
from ..AbstractRecommender import SeqAbstractRecommender

NO_HISTORY = "users without train items score b_j - |P_u + T - Q_j|, the query without a recent item (the reference " \
             "raises KeyError)"


class TransRec(SeqAbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(TransRec, self).__init__(dataset, conf)
        self.learning_rate = conf["learning_rate"]
        self.embedding_size = conf["embedding_size"]
        self.learner = conf["learner"]
        self.loss_function = conf["loss_function"]
        self.is_pairwise = conf["is_pairwise"]
        self.num_epochs = conf["epochs"]
        self.reg_mf = conf["reg_mf"]
        self.batch_size = conf["batch_size"]
        self.verbose = conf["verbose"]
        self.num_negatives = conf["num_neg"]
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.dataset = dataset
        self.train_matrix = dataset.train_matrix
        self.train_dict = dataset.get_user_train_dict(by_time=True)       # TransRec.py:41: csr_to_user_dict_bytime
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None
        self.last_items = None

    def build_graph(self):
        import torch
        from ...transrec import TransRecEngine
        require_single_gpu("TransRec")
        init = get_initializer(self.init_method, self.stddev, seed=2017)   # main.py:12
        P = init([self.num_users, self.embedding_size])                    # creation order of TransRec.py:56-64
        Q = init([self.num_items, self.embedding_size])
        b = init([self.num_items])
        T = init([1, self.embedding_size])
        self.engine = TransRecEngine(P, Q, b, T, self.learning_rate, self.reg_mf, self.batch_size,
                                     loss=self.loss_function, pairwise=self.is_pairwise is True, learner=self.learner)
        last = last_item_of(self.train_dict, self.num_users)               # TransRec.py:157: train_dict[u][-1]
        self.last_items = torch.from_numpy(last).to(self.engine.P.device)

    # ---------- training process -------
    def train_model(self):
        # TransRec.py:143-144: the reference's `[iter ...]` line is commented out; the figure is kept, not logged
        train_time_order_model(self, 1, self.is_pairwise is True, NO_HISTORY, log_loss=False)

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def predict(self, user_ids, candidate_items_userids=None):
        """Full mode: the [B, num_items] score rows as a device tensor (the evaluator's score-matrix path reads it in
        place).  Candidate mode: a list of per-user numpy arrays, the candidates' entries of those rows."""
        ratings = self.engine.score(np.asarray(list(user_ids), dtype=np.int32), self.last_items)
        if candidate_items_userids is None:
            return ratings
        host = ratings.cpu().numpy()
        return [host[k, np.asarray(items, dtype=np.int64)] for k, items in enumerate(candidate_items_userids)]
