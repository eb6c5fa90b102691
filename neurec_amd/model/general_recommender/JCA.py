"""JCA on the HIP engine.

Reference: Ziwei Zhu et al., "Improving Top-K Recommendation via Joint Collaborative Autoencoders." in WWW 2019.
Plugin-compatible with model/general_recommender/JCA.py: same constructor, config keys (conf/JCA.properties:
hidden_neuron, learning_rate, learner, reg, epochs, batch_size, verbose, f_act, g_act, margin, corruption_level,
init_method, stddev, num_neg), schedule, log lines (`metrics_info()` once, `[iter %d : loss : %f, time: %f]` per epoch,
`epoch %d:\\t%s` whenever epoch % verbose == 0) and `evaluate()` / `predict(users, items)`.  The pairs, the block step, the
optimiser sweep and the scorer are neurec_amd/jca.py (csrc/jca.hip); no dense [B, I] or [U, B] slab is formed.

As the reference:
  * `corruption_level` is read and never used;
  * `total_loss += loss` sits outside the inner loop (JCA.py:160): the logged loss is the sum over the row batches of
    the LAST column block's loss, and it is not divided;
  * `num_batch_U = int(num_users / batch_size) + 1`, and the same for the items: a count that is a multiple of
    batch_size gives an empty last batch;
  * the permutations of the users and of the items are drawn afresh each epoch (numpy's global stream, users first);
  * epochs run from 1;
  * `evaluate()` is computed from the whole matrix, with both index lists the identity;
  * `predict()` reads those ratings in both modes;
  * every variable is consumed by matmul, so the optimiser's dense form moves all of every variable at each block
    step: under Adam a row without a gradient still moves;
  * I_factor_vector is trained and not regularised.

Deviations, on purpose:
  * draws: the negatives are the device's counter-based ones, not `np.random.choice`: negative k of the positive at
    block cell (a, b) is a pure function of (seed, epoch, row batch i, column batch j, the cell, k, attempt);
  * initial values: numpy generators with fixed seeds, in the reference's creation order UV, UW, Ub1, Ub2, IV, IW, Ib1,
    Ib2, I_factor_vector (`init_method` tnormal / normal / uniform with `stddev`; the others fall to tnormal as in
    tool.get_initializer's last branch);
  * blocks without pairs: such a block is skipped — no optimiser step, loss 0.  The cases are an empty last batch and
    a block without a stored entry; the reference feeds an array of shape (0,) into a [None, 2] placeholder there, and
    TensorFlow raises;
  * rows short of unobserved columns: a block row with fewer than num_neg unobserved columns in the block contributes no
    pairs; `np.random.choice(..., replace=False)` raises there;
  * train-matrix values: a train matrix with a stored value other than 1 is refused, and the value is named; the
    reference would silently take only the entries equal to 1 as positives while feeding the ratings as input;
  * a pair whose hinge argument is exactly 0 is inactive (tf.maximum hands a tie's gradient to its first argument);
  * limits: hidden_neuron 1 to 128, batch_size 1 to 512, num_neg 1 to 8, f_act and g_act in {sigmoid, tanh, relu, elu,
    identity} (softmax needs the whole row and selu is left out; both are refused by name), learner in {adam, gd},
    margin >= 0, reg >= 0, learning_rate > 0; every refusal names the key and the supported range; multi-rank runs
    are refused;
  * return forms: predict() in full mode returns the [B, num_items] device tensor, in candidate mode per-user numpy
    arrays; no [num_users, num_items] rating matrix is kept: `evaluate()` refreshes the item codes [num_items, H] once
    and predict() scores its users against them.
"""
from time import time

import numpy as np

from .._common import require_single_gpu
from ..AbstractRecommender import AbstractRecommender

_ORDER = ("UV", "UW", "Ub1", "Ub2", "IV", "IW", "Ib1", "Ib2", "I_factor_vector")


def initial_variables(num_users, num_items, hidden_neuron, init_method="tnormal", stddev=0.01, seed=2019):
    """{name: float32 array} in the reference's creation order (JCA.py:55-78)"""
    rs = np.random.RandomState(seed)
    U, I, H = int(num_users), int(num_items), int(hidden_neuron)
    shapes = {"UV": (I, H), "UW": (H, I), "Ub1": (1, H), "Ub2": (1, I), "IV": (U, H), "IW": (H, U), "Ib1": (1, H),
              "Ib2": (1, U), "I_factor_vector": (1, I)}

    def draw(shape):
        if init_method == "uniform":
            return rs.uniform(-stddev, stddev, shape)
        x = rs.standard_normal(shape)
        if init_method != "normal":                           # truncated at two standard deviations, by redrawing
            bad = np.abs(x) > 2.0
            while bad.any():
                x[bad] = rs.standard_normal(int(bad.sum()))
                bad = np.abs(x) > 2.0
        return stddev * x
    return {k: draw(shapes[k]).astype(np.float32) for k in _ORDER}


class JCA(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(JCA, self).__init__(dataset, conf)
        self.hidden_neuron = conf["hidden_neuron"]
        self.learning_rate = conf["learning_rate"]
        self.learner = conf["learner"]
        self.reg = conf["reg"]
        self.num_epochs = conf["epochs"]
        self.batch_size = conf["batch_size"]
        self.verbose = conf["verbose"]
        self.f_act = conf["f_act"]
        self.g_act = conf["g_act"]
        self.margin = conf["margin"]
        self.corruption_level = conf["corruption_level"]      # read and never used, as in the reference
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.neg_sample_rate = conf["num_neg"]
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.dataset = dataset
        self.train_matrix = dataset.train_matrix.tocsr()
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...jca import JCAEngine, check_config, check_train_values
        require_single_gpu("JCA")
        check_config(self.hidden_neuron, self.batch_size, self.neg_sample_rate, self.f_act, self.g_act, self.learner,
                     self.margin, self.reg, self.learning_rate)
        check_train_values(self.train_matrix)
        self.num_batch_U = int(self.num_users / float(self.batch_size)) + 1
        self.num_batch_I = int(self.num_items / float(self.batch_size)) + 1
        self.engine = JCAEngine(initial_variables(self.num_users, self.num_items, self.hidden_neuron, self.init_method,
                                                  self.stddev), self.train_matrix, self.hidden_neuron, self.batch_size,
                                num_neg=self.neg_sample_rate, f_act=self.f_act, g_act=self.g_act, learner=self.learner,
                                learning_rate=self.learning_rate, reg=self.reg, margin=self.margin, seed=2019)

    def _batch(self, perm, k, n_batches):
        if k == n_batches - 1:
            return perm[k * self.batch_size:]
        return perm[k * self.batch_size:(k + 1) * self.batch_size]

    def train_model(self):
        import torch
        engine = self.engine
        self.logger.info(self.evaluator.metrics_info())
        self.num_batch_U = int(self.num_users / float(self.batch_size)) + 1
        self.num_batch_I = int(self.num_items / float(self.batch_size)) + 1
        self.block_losses = torch.zeros((self.num_batch_U, self.num_batch_I, 2), dtype=torch.float32, device=engine.dev)
        for epoch in range(1, self.num_epochs + 1):
            random_row_idx = np.random.permutation(self.num_users)
            random_col_idx = np.random.permutation(self.num_items)
            training_start_time = time()
            for i in range(self.num_batch_U):
                row_idx = self._batch(random_row_idx, i, self.num_batch_U)
                for j in range(self.num_batch_I):
                    col_idx = self._batch(random_col_idx, j, self.num_batch_I)
                    pairs = engine.pairs(row_idx, col_idx, epoch, i, j)
                    engine.step(row_idx, col_idx, pairs, self.block_losses[i, j])
            total_loss = 0.0                                  # `total_loss += loss` after the inner loop (JCA.py:160)
            for hinge, regl in self.block_losses[:, self.num_batch_I - 1].cpu().numpy():
                total_loss += np.float32(hinge) + np.float32(regl)
            self.logger.info("[iter %d : loss : %f, time: %f]" % (epoch, total_loss, time() - training_start_time))
            if epoch % self.verbose == 0:
                self.logger.info("epoch %d:\t%s" % (epoch, self.evaluate()))

    def evaluate(self):
        self.engine.encode_items()
        return self.evaluator.evaluate(self)

    def predict(self, user_ids, candidate_items_user_ids=None):
        """Full mode: the [B, num_items] score rows as a device tensor.  Candidate mode: a list of per-user numpy
        arrays."""
        users = np.asarray(list(user_ids), dtype=np.int32)
        if candidate_items_user_ids is None:
            return self.engine.score(users)
        sizes = [len(its) for its in candidate_items_user_ids]
        if not sizes:
            return []
        flat = np.concatenate([np.asarray(its, dtype=np.int32).reshape(-1) for its in candidate_items_user_ids])
        out = self.engine.score_pairs(np.repeat(users, sizes), flat).cpu().numpy()
        return np.split(out, np.cumsum(sizes)[:-1])
