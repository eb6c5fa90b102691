"""NPE on the HIP engine.

Reference: ThaiBinh Nguyen et al., "NPE: Neural Personalized Embedding for Collaborative Filtering." IJCAI 2018.
Plugin-compatible with model/sequential_recommender/NPE.py: same constructor, config keys (conf/NPE.properties: epochs,
batch_size, embedding_size, reg, learning_rate, learner, high_order, num_neg, loss_function, init_method, stddev,
verbose), log lines and `predict` contract.  The per-batch `sess.run((loss, optimizer))` is neurec_amd/npe.py
(csrc/npe.hip); the instances come from the device stream of the time-order pointwise sampler at high_order = L, its
`recent` field as it comes (oldest first).

Deviations, on purpose:
(a) A user without train items scores <relu(P_u), relu(V_i)>: its context is empty (the reference raises KeyError).
(b) At high_order = 1 the reference's sampler yields 1-D recents (data/sampler.py:60-61) and the graph's rank-2
    placeholder `item_input_recent` ([None, None], NPE.py:41) cannot take them: the reference does not train.  Here
    L = 1 is a context of one item, in training and in predict().
Kept: predict() slices `seq[len(seq) - L:]`, so a user with 0 < |R_u| < L has the context of its last
min(L - |R_u|, |R_u|) items.  Candidate mode returns the candidates' entries of the full-mode rows.
"""
from ...util import timer
from ...util.tool import get_initializer
from ..AbstractRecommender import SeqAbstractRecommender
from .._common import predict_scores, require_single_gpu, train_time_order_model
from .HRM import last_items_table

DEVIATIONS = "users without train items score <relu(P_u), relu(V_i)> (the reference raises KeyError); at " \
             "high_order = 1 the context is the one last item, in training and in predict() (the reference's rank-2 " \
             "placeholder cannot take the sampler's 1-D recents); kept: users with fewer than high_order train items " \
             "have the context of their last min(L - |R_u|, |R_u|)"


class NPE(SeqAbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(NPE, self).__init__(dataset, conf)
        self.learning_rate = conf["learning_rate"]
        self.embedding_size = conf["embedding_size"]
        self.learner = conf["learner"]
        self.loss_function = conf["loss_function"]
        self.num_epochs = conf["epochs"]
        self.reg = conf["reg"]
        self.batch_size = conf["batch_size"]
        self.high_order = conf["high_order"]
        self.verbose = conf["verbose"]
        self.num_negatives = conf["num_neg"]
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.dataset = dataset
        self.train_dict = dataset.get_user_train_dict(by_time=True)       # NPE.py:34: csr_to_user_dict_bytime
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None
        self.last_items = None

    def build_graph(self):
        from ...npe import NPEEngine
        require_single_gpu("NPE")
        init = get_initializer(self.init_method, self.stddev, seed=2017)   # main.py:12
        P = init([self.num_users, self.embedding_size])                    # creation order of NPE.py:47-52
        V = init([self.num_items, self.embedding_size])
        W = init([self.num_items, self.embedding_size])
        last = last_items_table(self.train_dict, self.num_users, self.high_order)
        self.engine = NPEEngine(P, V, W, self.learning_rate, self.reg, self.batch_size, self.high_order,
                                loss=self.loss_function, learner=self.learner, last_items=last)
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
        """Device tables for the evaluator's on-GPU factor path: h_u against relu(V)."""
        return self.engine.eval_factors()

    def predict(self, user_ids, candidate_items_userids=None):
        P, Q = self.engine.eval_factors()
        return predict_scores(P, Q, user_ids, candidate_items_userids)
