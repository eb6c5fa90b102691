"""MLP on the HIP engine: the MLP half of Neural Collaborative Filtering.

Reference: Xiangnan He et al., "Neural Collaborative Filtering." in WWW 2017.
Plugin-compatible with model/general_recommender/MLP.py: same constructor, config keys (conf/MLP.properties: epochs,
batch_size, layers, reg_mlp, learning_rate, learner, is_pairwise, num_neg, loss_function, verbose, init_method, stddev),
log lines and `predict` contract.  It is NeuMF without the two mf_* tables and with reg_mlp only: the score is
sum(h_last).  The engine is neurec_amd/neumf.py at embedding_size 0 (csrc/neumf.hip).

As the reference: a fresh sampler in every epoch (NeuMF makes one before the first); evaluate() is not timed.

Deviations, on purpose:
  * `is_pairwise=True` is refused, and the shipped conf/MLP.properties sets it: run with `--is_pairwise=False
    --loss_function=cross_entropy` (or square).  The step kernel scores one item per instance; pairwise mode for both
    models is left for a later change, together with NeuMF's (whose reference graph does not even share the layer stack
    between the two items — see model/general_recommender/NeuMF.py).
  * the instances come from the device `PointwiseSampler` stream (epoch k's sampler is seeded 2018 + k), the initial
    values from numpy generators seeded 2017; multi-rank runs are refused; predict() in full mode returns the device
    tensor, in candidate mode per-user numpy arrays.
"""
from ..AbstractRecommender import AbstractRecommender
from .._common import require_single_gpu
from .NeuMF import initial_variables, predict_pairs, train_pointwise_model


class MLP(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(MLP, self).__init__(dataset, conf)
        self.layers = conf["layers"]
        self.learning_rate = conf["learning_rate"]
        self.is_pairwise = conf["is_pairwise"]
        self.learner = conf["learner"]
        self.num_epochs = conf["epochs"]
        self.num_negatives = conf["num_neg"]
        self.reg_mlp = conf["reg_mlp"]
        self.batch_size = conf["batch_size"]
        self.loss_function = conf["loss_function"]
        self.verbose = conf["verbose"]
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.dataset = dataset
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...neumf import NeuMFEngine, check_shape
        require_single_gpu("MLP")
        if self.is_pairwise is True:
            raise NotImplementedError(
                "MLP: is_pairwise=True is not supported (the shipped conf/MLP.properties sets it): the step scores one "
                "item per instance and pairwise mode is not built; run with is_pairwise=False and a pointwise "
                "loss_function (cross_entropy, square)")
        layers = check_shape("MLP", 0, self.layers)
        variables = initial_variables(self.num_users, self.num_items, 0, layers, self.init_method, self.stddev,
                                      with_mf=False)
        self.engine = NeuMFEngine(variables, layers, self.learning_rate, 0.0, self.reg_mlp, self.batch_size,
                                  loss=self.loss_function, learner=self.learner, name="MLP")

    def train_model(self):
        train_pointwise_model(self, sampler_per_epoch=True)

    def evaluate(self):
        return self.evaluator.evaluate(self)

    def predict(self, user_ids, candidate_items_userids=None):
        """Full mode: the [B, num_items] score rows as a device tensor.  Candidate mode: per-user numpy arrays."""
        return predict_pairs(self.engine, user_ids, candidate_items_userids)
