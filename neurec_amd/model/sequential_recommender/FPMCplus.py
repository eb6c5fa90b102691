"""FPMCplus on the HIP engine.

FPMC (Steffen Rendle et al., "Factorizing Personalized Markov Chains for Next-Basket Recommendation." WWW 2010) with an
attention MLP over the user's last high_order items, per target item.
Plugin-compatible with model/sequential_recommender/FPMCplus.py: same constructor, config keys (conf/FPMCplus.properties:
epochs, batch_size, embedding_size, weight_size, high_order, reg_mf, reg_w, learning_rate, learner, is_pairwise, num_neg,
loss_function, embed_init_method, weight_init_method, stddev, verbose), log lines and `predict` contract.  The per-batch
`sess.run((loss, optimizer))` is neurec_amd/fpmcplus.py (csrc/fpmcplus.hip); the instances come from the device stream
of the time-order samplers at high_order = L.

Kept, as the class has them: pointwise mode has no reg_w term; b is never regularised; h starts as ones; W, b and h get
the dense optimiser application every step, the four tables the sparse one; the logged loss is divided by the number
of batches.

Deviations, on purpose:
(a) A user without train items scores <UI_u, IU_i> (the reference raises KeyError).
(b) A user with 0 < |R_u| < L: predict() feeds a slice shorter than L into a concat with two [N, L, d] operands and the
    reference fails.  Here the attention runs over the user's last min(|R_u|, L) items, the softmax over those alone.
(c) At high_order = 1 the reference's sampler yields 1-D recents that the rank-2 placeholder `item_input_recent`
    cannot take.  Here L = 1 trains and scores: alpha = 1, the model is FPMC, and W, b, h move by the regulariser alone.
Candidate mode returns the candidates' entries of the full-mode rows.
"""
import numpy as np

from ...util import timer
from ...util.tool import get_initializer
from .._common import last_items_table, require_single_gpu, train_time_order_model
from ..AbstractRecommender import SeqAbstractRecommender

DEVIATIONS = "users without train items score <UI_u, IU_i> (the reference raises KeyError); users with fewer than " \
             "high_order train items attend over the items they have, the softmax over those alone (the reference's " \
             "concat fails on the short slice); at high_order = 1 the one last item has weight 1, in training and in " \
             "predict() (the reference's rank-2 placeholder cannot take the sampler's 1-D recents)"


class FPMCplus(SeqAbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(FPMCplus, self).__init__(dataset, conf)
        self.learning_rate = conf["learning_rate"]
        self.embedding_size = conf["embedding_size"]
        self.weight_size = conf["weight_size"]
        self.learner = conf["learner"]
        self.loss_function = conf["loss_function"]
        self.is_pairwise = conf["is_pairwise"]
        self.num_epochs = conf["epochs"]
        self.reg_mf = conf["reg_mf"]
        self.reg_w = conf["reg_w"]
        self.batch_size = conf["batch_size"]
        self.high_order = conf["high_order"]
        self.verbose = conf["verbose"]
        self.embed_init_method = conf["embed_init_method"]
        self.weight_init_method = conf["weight_init_method"]
        self.stddev = float(conf["stddev"])
        self.num_negatives = conf["num_neg"]
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.dataset = dataset
        self.train_matrix = dataset.train_matrix
        self.train_dict = dataset.get_user_train_dict(by_time=True)       # FPMCplus.py:40: csr_to_user_dict_bytime
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...fpmcplus import FPMCplusEngine
        require_single_gpu("FPMCplus")
        d, w = self.embedding_size, self.weight_size
        embed_init = get_initializer(self.embed_init_method, self.stddev, seed=2017)   # main.py:12
        UI = embed_init([self.num_users, d])                   # creation order of FPMCplus.py:58-71
        IU = embed_init([self.num_items, d])
        IL = embed_init([self.num_items, d])
        LI = embed_init([self.num_items, d])
        weight_init = get_initializer(self.weight_init_method, self.stddev, seed=2017)
        W = weight_init([3 * d, w])
        b = weight_init([1, w])
        h = np.ones([w, 1], np.float32)
        last = last_items_table(self.train_dict, self.num_users, self.high_order)
        self.engine = FPMCplusEngine(UI, IU, IL, LI, W, b, h, self.learning_rate, self.reg_mf, self.reg_w,
                                     self.batch_size, self.high_order, loss=self.loss_function,
                                     pairwise=self.is_pairwise is True, learner=self.learner, last_items=last)

    # ---------- training process -------
    def train_model(self):
        engine, L = self.engine, self.high_order
        train_time_order_model(self, L, self.is_pairwise is True, DEVIATIONS,
                               step=lambda u, recent, i, t, out: engine.step(u, recent.reshape(-1, L), i, t, out))

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def predict(self, user_ids, candidate_items_userids=None):
        """Full mode: the [B, num_items] score rows as a device tensor (the evaluator's score-matrix path reads it in
        place).  Candidate mode: a list of per-user numpy arrays, the candidates' entries of those rows."""
        ratings = self.engine.score(np.asarray(list(user_ids), dtype=np.int32))
        if candidate_items_userids is None:
            return ratings
        host = ratings.cpu().numpy()
        return [host[k, np.asarray(items, dtype=np.int64)] for k, items in enumerate(candidate_items_userids)]
