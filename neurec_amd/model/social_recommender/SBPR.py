"""SBPR on the HIP engine.

Reference: Tong Zhao et al., "Leveraging Social Connections to Improve Personalized Ranking for Collaborative
Filtering." in CIKM 2014.
Plugin-compatible with model/social_recommender/SBPR.py: same constructor, config keys (conf/SBPR.properties:
learning_rate, embedding_size, learner, loss_function, num_epochs, reg_mf, batch_size, social_file, init_method, stddev,
verbose), log lines and `predict` contract.  The social item sets (_get_SocialItemsSet), the instances of an epoch
(_get_pairwise_all_data and the DataIterator's permutation) and the per-batch `sess.run((loss, optimizer))` are
neurec_amd/sbpr.py (csrc/sbpr.hip): nothing of an epoch passes through the host but its loss figures.

Kept, as the class has them: the trust matrix is directed and used as given; the number of epochs is `num_epochs` and
the loop runs from 0 (`epoch % verbose == 0`); the logged figure is total_loss / the number of INSTANCES; users without
a social item never train; predict() ranks by P_u . Q_j WITHOUT the bias that training uses.

Deviation, on purpose:
  - a trusted user without train items contributes nothing to the social sets (the reference raises KeyError in
    _get_SocialItemsSet);
  - an eligible user whose train items and social items are all the items is refused with a ValueError naming the user
    when the sets are built (the reference divides by zero inside randint_choice);
  - the trust file's ids and the keys of dataset.userids are compared in their string form (the reference's np.in1d
    keeps nothing when one side is strings and the other integers).
The draws are the device's counter-based ones, not numpy's global stream: the same laws, not the same numbers.
"""
from time import time

from ...util import timer
from ...util.tool import get_initializer
from .._common import predict_scores, require_single_gpu
from ..AbstractRecommender import SocialAbstractRecommender

DEVIATIONS = "trusted users without train items add nothing to the social sets (the reference raises KeyError); " \
             "trust ids and user ids are compared as strings"


class SBPR(SocialAbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(SBPR, self).__init__(dataset, conf)
        self.learning_rate = conf["learning_rate"]
        self.embedding_size = conf["embedding_size"]
        self.learner = conf["learner"]
        self.loss_function = conf["loss_function"]
        self.num_epochs = conf["num_epochs"]
        self.reg_mf = conf["reg_mf"]
        self.batch_size = conf["batch_size"]
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.verbose = conf["verbose"]
        self.dataset = dataset
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.userids = self.dataset.userids
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...sbpr import SBPREngine
        require_single_gpu("SBPR")
        init = get_initializer(self.init_method, self.stddev, seed=2017)   # main.py:12
        P = init([self.num_users, self.embedding_size])                    # creation order of SBPR.py:59-66
        Q = init([self.num_items, self.embedding_size])
        b = init([self.num_items])
        self.engine = SBPREngine(P, Q, b, self.dataset.train_matrix, self.social_matrix, self.learning_rate,
                                 self.reg_mf, self.batch_size, loss=self.loss_function, learner=self.learner)

    # ---------- training process -------
    def train_model(self):
        self.logger.info(self.evaluator.metrics_info())
        self.logger.info(DEVIATIONS)
        self.epoch_losses = []
        for epoch in range(self.num_epochs):
            training_start_time = time()
            total_loss, num_training_instances = self.engine.train_epoch(epoch, self.batch_size)
            self.epoch_losses.append(total_loss / max(num_training_instances, 1))
            self.logger.info("[iter %d : loss : %f, time: %f]" % (epoch, self.epoch_losses[-1],
                                                                 time() - training_start_time))
            if epoch % self.verbose == 0:
                self.logger.info("epoch %d:\t%s" % (epoch, self.evaluate()))

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def get_eval_factors(self):
        """Device tables for the evaluator's on-GPU factor path: the score is P_u . Q_j, no bias"""
        return self.engine.P, self.engine.Q

    def predict(self, user_ids, candidate_items_userids=None):
        return predict_scores(self.engine.P, self.engine.Q, user_ids, candidate_items_userids)
