"""DeepICF on the HIP engine.

Reference: Feng Xue et al., "Deep Item-based Collaborative Filtering for Top-N Recommendation." TOIS 2019.
Plugin-compatible with model/general_recommender/DeepICF.py: same constructor, config keys (conf/DeepICF.properties:
pretrain_file, verbose, learner, batch_size, epochs, layers, weight_size, embedding_size, data_alpha, regs, regw, alpha,
beta, num_neg, learning_rate, activation, algorithm, batch_norm, embed_init_method, weight_init_method,
bias_init_method, stddev), log lines and `predict` contract.  The per-batch `sess.run((loss, optimizer))` on histories
padded to [B, Lmax] and the per-user `sess.run` of predict() are neurec_amd/deepicf.py (csrc/deepicf.hip).

As the reference: the exponent of num_idx is +alpha; `data_alpha` and `pretrain_file` are read and never used
(`self.mlp_pretrain` does not exist, so build_graph always ends in "load pretrained params unsuccessful!");
`activation` selects relu / sigmoid / tanh only as the int 0 / 1 / 2 — the shipped `activation=Relu` applies none; the
attention's mask covers one padding row for every instance shorter than the longest of its batch
(`--attention_mask=history`, not a reference key, gives the softmax over the history alone); `biases['b%d']` and
`biases['out']` start from a normal draw of stddev 1; the instances are the pointwise FISM-style stream (there is no
pairwise mode); the moving variance takes Bessel's correction, the normalisation does not.

Deviations, on purpose: predict() reads the moving statistics and changes nothing — the reference builds both
batch-norm branches outside tf.cond, so its predict() also runs the training branch and shifts the moving statistics,
in an order relative to the inference branch's read that the graph leaves open; the gradient of a pre-norm bias under
batch norm, zero in exact arithmetic, is written as exact zeros (the reference's Adam amplifies its rounding noise);
and NAIS's: a user without train items scores through an empty pooling (the reference raises KeyError); the instances
come from the device streams; multi-rank runs are refused; candidate mode returns the candidates' entries of the
full-mode rows.
"""
import numpy as np

from ...util import timer
from ...util.tool import get_initializer
from ..AbstractRecommender import AbstractRecommender
from .._common import require_single_gpu, train_history_model


class DeepICF(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(DeepICF, self).__init__(dataset, conf)
        self.pretrain_file = conf["pretrain_file"]
        self.verbose = conf["verbose"]
        self.batch_size = conf["batch_size"]
        self.use_batch_norm = conf["batch_norm"]
        self.num_epochs = conf["epochs"]
        self.weight_size = conf["weight_size"]
        self.embedding_size = conf["embedding_size"]
        self.n_hidden = conf["layers"]
        regs = conf["regs"]
        self.reg_W = conf["regw"]
        self.lambda_bilinear = regs[0]
        self.gamma_bilinear = regs[1]
        self.eta_bilinear = regs[2]
        self.alpha = conf["alpha"]
        self.beta = conf["beta"]
        self.num_negatives = conf["num_neg"]
        self.learning_rate = conf["learning_rate"]
        self.activation = conf["activation"]
        self.algorithm = conf["algorithm"]
        self.learner = conf["learner"]
        self.embed_init_method = conf["embed_init_method"]
        self.weight_init_method = conf["weight_init_method"]
        self.bias_init_method = conf["bias_init_method"]
        self.stddev = conf["stddev"]
        # not keys of the reference
        self.attention_mask = conf["attention_mask"] if "attention_mask" in conf else "reference"
        self.is_pairwise = False              # train_history_model's switch: DeepICF has the pointwise stream alone
        self.dataset = dataset
        self.num_items = dataset.num_items
        self.num_users = dataset.num_users
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...deepicf import DeepICFEngine, check_layers
        from ...nais import ACTIVATIONS, MAX_D, MAX_W, activation_code
        require_single_gpu("DeepICF")
        d, w = self.embedding_size, self.weight_size
        layers = check_layers(list(self.n_hidden))
        if d < 1 or d > MAX_D:
            raise NotImplementedError("DeepICF: embedding_size=%d is not supported (1 to %d)" % (d, MAX_D))
        if w < 1 or w > MAX_W:
            raise NotImplementedError("DeepICF: weight_size=%d is not supported (1 to %d)" % (w, MAX_W))
        if not float(self.beta) >= 0.0:
            raise ValueError("DeepICF needs beta >= 0, got %r" % (self.beta,))
        # DeepICF.py:186-195: self.mlp_pretrain does not exist, so the try block always fails; nothing is loaded
        self.logger.info("load pretrained params unsuccessful!")
        self.logger.info("activation: %s" % ACTIVATIONS.get(activation_code(self.activation),
                                                            "none (activation=%r is not 0, 1 or 2)" % (self.activation,)))
        self.logger.info("attention mask: %s" % ("reference (num_idx = |H| + 1: one padding row for histories shorter "
                                                 "than the batch's longest)" if self.attention_mask == "reference"
                                                 else "history (the softmax over the history alone)"))
        embed_init = get_initializer(self.embed_init_method, self.stddev, seed=2017)
        c1 = embed_init([self.num_items, d])
        Q = embed_init([self.num_items, d])
        weight_init = get_initializer(self.weight_init_method, self.stddev, seed=2017)
        bias_init = get_initializer(self.bias_init_method, self.stddev, seed=2017)
        W = weight_init([(self.algorithm + 1) * d, w])
        b = bias_init([1, w])
        rs = np.random.RandomState(2017)
        tower = {"Wout": weight_init([layers[-1], 1]), "bout": rs.randn(1).astype(np.float32)}
        n_in = d
        for k, n in enumerate(layers):
            tower["W%d" % k] = weight_init([n_in, n])
            tower["b%d" % k] = rs.randn(n).astype(np.float32)          # tf.random_normal([n]): stddev 1
            n_in = n
        self.engine = DeepICFEngine(c1, Q, W, b, tower, self.dataset.train_matrix, self.learning_rate,
                                    [self.lambda_bilinear, self.gamma_bilinear, self.eta_bilinear], list(self.reg_W),
                                    self.alpha, self.beta, self.batch_size, algorithm=self.algorithm,
                                    activation=self.activation, batch_norm=bool(self.use_batch_norm),
                                    learner=self.learner, attention_mask=self.attention_mask)

    # ---------- training process -------
    def train_model(self):
        # the epoch's largest batch in history positions: one scalar copy, and the gradient buffer is sized to it
        train_history_model(self, before_batches=lambda batches: {
            "positions": self.engine.max_positions([b[0] for b in batches])}, after_epoch=self.engine.verify)

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
