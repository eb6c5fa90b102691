"""ItemKNN (item-based nearest neighbours) on the HIP engine.

Reference: https://github.com/MaurizioFD/RecSys2019_DeepLearning_Evaluation (the similarity classes the reference's
model/general_recommender/ItemKNN.py carries).
Plugin-compatible with that file: same constructor, config keys (conf/ItemKNN.properties: neighbor, shrink, similarity,
asymmetric_alpha, tversky_alpha, tversky_beta, verbose), log lines and `predict` contract.  The reference's per-column
Python loop and its dense U x I `ratings` matrix are the on-device build and the per-batch scoring of
neurec_amd/itemknn.py; there is nothing to train.

Deviations, on purpose: among equal similarities the lower item index is kept (the reference keeps whatever
`argpartition` leaves); with `similarity=euclidean` a pair of items without interactions scores 0 where the reference
computes 0/0; `neighbor` is at most 1,024 (the properties file names 5 to 800).  Candidate mode, which the reference
leaves "waiting to complete", returns the candidates' entries of the same score rows.
"""
import numpy as np

from ...util import timer
from .._common import require_single_gpu
from ..AbstractRecommender import AbstractRecommender


class ItemKNN(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(ItemKNN, self).__init__(dataset, conf)
        self.verbose = conf["verbose"]
        self.topK = conf["neighbor"]
        self.shrink = conf["shrink"]
        self.dataset = dataset
        self.train_matrix = self.dataset.train_matrix
        self.similarity = conf["similarity"]
        self.asymmetric_alpha = conf["asymmetric_alpha"]
        self.tversky_alpha = conf["tversky_alpha"]
        self.tversky_beta = conf["tversky_beta"]
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...itemknn import ItemKNNEngine
        require_single_gpu("ItemKNN")
        self.engine = ItemKNNEngine(self.train_matrix, self.topK, self.shrink, self.similarity,
                                    self.asymmetric_alpha, self.tversky_alpha, self.tversky_beta)

    def train_model(self):
        self.logger.info(self.evaluator.metrics_info())
        self.logger.info(self.evaluate())

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def predict(self, user_ids, candidate_items=None):
        """Full mode: the [B, num_items] score rows as a device tensor (the evaluator's score-matrix path reads it in
        place).  Candidate mode: a list of per-user numpy arrays, the candidates' entries of those rows."""
        ratings = self.engine.score(np.asarray(list(user_ids), dtype=np.int32))
        if candidate_items is None:
            return ratings
        host = ratings.cpu().numpy()
        return [host[k, np.asarray(items, dtype=np.int64)] for k, items in enumerate(candidate_items)]
