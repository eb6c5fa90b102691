"""FISM on the HIP engine.

Reference: Santosh Kabbur et al., "FISM: Factored Item Similarity Models for Top-N Recommender Systems." KDD 2013.
Plugin-compatible with model/general_recommender/FISM.py: same constructor, config keys (conf/FISM.properties:
batch_size, epochs, embedding_size, regs, alpha, num_neg, learning_rate, learner, topk, loss_function, is_pairwise,
init_method, stddev, verbose), log lines and `predict` contract.  The per-batch `sess.run((loss, optimizer))` on
histories padded to [B, Lmax] is neurec_amd/fism.py (csrc/fism.hip); the instances come from the device streams
(PointwiseSampler / PairwiseSampler), not from the reference's numpy generator.

Deviations, on purpose: the reference's pairwise generator (_get_pairwise_all_likefism_data) hands the graph an empty
history for every instance, so that only the bias trains; pairwise mode here uses the structure its pointwise
generator states (positive side: the history without the item, n = |R_u|; negative side: the whole history,
n = |R_u| + 1; users with one train item take no part).  A user without train items scores `bias` alone (the
reference raises KeyError).  Candidate mode returns the candidates' entries of the full-mode rows.
"""
from ...util import timer
from ...util.tool import get_initializer
from ..AbstractRecommender import AbstractRecommender
from .._common import predict_scores, require_single_gpu, train_history_model


class FISM(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(FISM, self).__init__(dataset, conf)
        self.batch_size = conf["batch_size"]
        self.num_epochs = conf["epochs"]
        self.embedding_size = conf["embedding_size"]
        self.regs = conf["regs"]
        self.lambda_bilinear = self.regs[0]
        self.gamma_bilinear = self.regs[1]
        self.alpha = conf["alpha"]
        self.num_negatives = conf["num_neg"]
        self.learning_rate = conf["learning_rate"]
        self.learner = conf["learner"]
        self.topK = conf["topk"]
        self.loss_function = conf["loss_function"]
        self.is_pairwise = conf["is_pairwise"]
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.verbose = conf["verbose"]
        # not a key of the reference: "rows" applies c1 by rows like Q and bias (neurec_amd/fism.py)
        self.c1_application = conf["c1_application"] if "c1_application" in conf else "dense"
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.dataset = dataset
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...fism import FISMEngine
        require_single_gpu("FISM")
        init = get_initializer(self.init_method, self.stddev, seed=2017)   # main.py:12
        c1 = init([self.num_items, self.embedding_size])
        Q = init([self.num_items, self.embedding_size])
        self.engine = FISMEngine(c1, Q, self.dataset.train_matrix, self.learning_rate, self.regs, self.alpha,
                                 self.batch_size, loss=self.loss_function, pairwise=self.is_pairwise is True,
                                 learner=self.learner, c1_application=self.c1_application)

    # ---------- training process -------
    def train_model(self):
        train_history_model(self)

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def get_eval_factors(self):
        """Device tables for the evaluator's on-GPU factor path: [|R_u|^-alpha p_u | 1] against [Q | bias]."""
        return self.engine.eval_factors()

    def predict(self, user_ids, candidate_items_userids=None):
        P, Q = self.engine.eval_factors()
        return predict_scores(P, Q, user_ids, candidate_items_userids)
