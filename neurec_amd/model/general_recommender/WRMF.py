"""WRMF (implicit-feedback ALS) on the HIP engine.

Reference: Yifan Hu et al., "Collaborative Filtering for Implicit Feedback Datasets." ICDM 2008.
Plugin-compatible with model/general_recommender/WRMF.py: same constructor, config keys (conf/WRMF.properties),
training loop, log lines and `predict` contract.  The reference's per-row `sess.run(update_user)` /
`sess.run(update_item)` loops (one solve per user, then one per item, against dense U x I matrices Cui / Pui) are one
batched on-device solve per side (neurec_amd/wrmf.py); the train matrix stays sparse.

One deviation: reg_mf must be > 0 (the solves factor an SPD matrix); the reference also accepts 0 whenever
Y^T Y happens to be full rank.
"""
from time import time

from ...util import timer
from ...util.tool import get_initializer
from ..AbstractRecommender import AbstractRecommender
from .._common import predict_scores, require_single_gpu


class WRMF(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(WRMF, self).__init__(dataset, conf)
        self.embedding_size = conf["embedding_size"]
        self.alpha = conf["alpha"]
        self.topK = conf["topk"]
        self.num_epochs = conf["epochs"]
        self.reg_mf = conf["reg_mf"]
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.verbose = conf["verbose"]
        self.dataset = dataset
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...wrmf import WRMFEngine
        require_single_gpu("WRMF")
        init = get_initializer(self.init_method, self.stddev, seed=2017)   # main.py:12
        users = init([self.num_users, self.embedding_size])
        items = init([self.num_items, self.embedding_size])
        self.engine = WRMFEngine(users, items, self.dataset.train_matrix, self.alpha, self.reg_mf)

    # ---------- training process -------
    def train_model(self):
        import torch
        self.logger.info(self.evaluator.metrics_info())
        for epoch in range(1, self.num_epochs + 1):
            training_start_time = time()
            print('solving for user vectors...')
            self.engine.solve_users()
            print('solving for item vectors...')
            self.engine.solve_items()
            torch.cuda.current_stream().synchronize()
            self.logger.info('iteration %i finished in %f seconds' % (epoch, time() - training_start_time))
            if epoch % self.verbose == 0:
                self.logger.info("epoch %d:\t%s" % (epoch, self.evaluate()))

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def get_eval_factors(self):
        """Device tables for the evaluator's on-GPU factor path: scores are P Q^T, as in MF."""
        return self.engine.P, self.engine.Q

    def predict(self, user_ids, candidate_items_userids=None):
        return predict_scores(self.engine.P, self.engine.Q, user_ids, candidate_items_userids)
