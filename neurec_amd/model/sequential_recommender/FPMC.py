"""FPMC on the HIP engine.

Reference: Steffen Rendle et al., "Factorizing Personalized Markov Chains for Next-Basket Recommendation." WWW 2010.
Plugin-compatible with model/sequential_recommender/FPMC.py: same constructor, config keys (conf/FPMC.properties:
epochs, batch_size, embedding_size, reg_mf, learning_rate, learner, is_pairwise, num_neg, loss_function, init_method,
stddev, verbose, topk), log lines and `predict` contract.  The per-batch `sess.run((loss, optimizer))` is
neurec_amd/fpmc.py (csrc/fpmc.hip); the instances come from the device streams of the time-order samplers at
high_order = 1.

Deviation, on purpose: a user without train items scores <UI_u, IU_i> alone (the reference raises KeyError).
Candidate mode returns the candidates' entries of the full-mode rows.
"""
from ...util import timer
from ...util.tool import get_initializer
from ..AbstractRecommender import SeqAbstractRecommender
from .._common import last_item_of, predict_scores, require_single_gpu, train_time_order_model

NO_HISTORY = "users without train items score <UI_u, IU_i> alone (the reference raises KeyError)"


class FPMC(SeqAbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(FPMC, self).__init__(dataset, conf)
        self.learning_rate = conf["learning_rate"]
        self.embedding_size = conf["embedding_size"]
        self.learner = conf["learner"]
        self.loss_function = conf["loss_function"]
        self.is_pairwise = conf["is_pairwise"]
        self.topK = conf["topk"]
        self.num_epochs = conf["epochs"]
        self.reg_mf = conf["reg_mf"]
        self.batch_size = conf["batch_size"]
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.verbose = conf["verbose"]
        self.num_negatives = conf["num_neg"]
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.dataset = dataset
        self.train_matrix = dataset.train_matrix
        self.train_dict = dataset.get_user_train_dict(by_time=True)
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None
        self.last_items = None

    def build_graph(self):
        import torch
        from ...fpmc import FPMCEngine
        require_single_gpu("FPMC")
        init = get_initializer(self.init_method, self.stddev, seed=2017)   # main.py:12
        UI = init([self.num_users, self.embedding_size])                   # creation order of FPMC.py:52-59
        IU = init([self.num_items, self.embedding_size])
        IL = init([self.num_items, self.embedding_size])
        LI = init([self.num_items, self.embedding_size])
        self.engine = FPMCEngine(UI, IU, IL, LI, self.learning_rate, self.reg_mf, self.batch_size,
                                 loss=self.loss_function, pairwise=self.is_pairwise is True, learner=self.learner)
        last = last_item_of(self.train_dict, self.num_users)               # FPMC.py:145-146: cand_items[-1]
        self.last_items = torch.from_numpy(last).to(self.engine.UI.device)

    # ---------- training process -------
    def train_model(self):
        train_time_order_model(self, 1, self.is_pairwise is True, NO_HISTORY)

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def get_eval_factors(self):
        """Device tables for the evaluator's on-GPU factor path: [UI_u | LI_last(u)] against [IU | IL]."""
        return self.engine.eval_factors(self.last_items)

    def predict(self, user_ids, candidate_items_userids=None):
        P, Q = self.engine.eval_factors(self.last_items)
        return predict_scores(P, Q, user_ids, candidate_items_userids)
