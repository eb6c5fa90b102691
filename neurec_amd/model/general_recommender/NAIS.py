"""NAIS on the HIP engine.

Reference: Xiangnan He et al., "NAIS: Neural Attentive Item Similarity Model for Recommendation." TKDE 2018.
Plugin-compatible with model/general_recommender/NAIS.py: same constructor, config keys (conf/NAIS.properties:
pretrain, verbose, learner, batch_size, epochs, weight_size, embedding_size, data_alpha, regs, alpha, beta, num_neg,
learning_rate, activation, algorithm, is_pairwise, loss_function, embed_init_method, weight_init_method, stddev,
pretrain_file), log lines and `predict` contract.  The per-batch `sess.run((loss, optimizer))` on histories padded to
[B, Lmax] and the per-user `sess.run` of predict() are neurec_amd/nais.py (csrc/nais.hip).

As the reference: the exponent of num_idx is +alpha; `regs[2]`, `data_alpha`, `pretrain` and `pretrain_file` are read
and never used (build_graph always ends in "load pretrained params unsuccessful!"); `activation` selects relu /
sigmoid / tanh only as the int 0 / 1 / 2 — the shipped `activation=Relu` applies none; the attention's mask covers one
padding row for every instance shorter than the longest of its side of the batch (`--attention_mask=history`, not a
reference key, gives the softmax over the history alone).

Deviations, on purpose, FISM's: pairwise mode uses the structure the pointwise generator states (the reference's
pairwise generator feeds empty histories); a user without train items scores `bias` alone (the reference raises
KeyError); the instances come from the device streams; multi-rank runs are refused; candidate mode returns the
candidates' entries of the full-mode rows.
"""
import numpy as np

from ...util import timer
from ...util.tool import get_initializer
from ..AbstractRecommender import AbstractRecommender
from .._common import require_single_gpu, train_history_model


class NAIS(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(NAIS, self).__init__(dataset, conf)
        self.pretrain = conf["pretrain"]
        self.verbose = conf["verbose"]
        self.batch_size = conf["batch_size"]
        self.num_epochs = conf["epochs"]
        self.weight_size = conf["weight_size"]
        self.embedding_size = conf["embedding_size"]
        self.data_alpha = conf["data_alpha"]
        self.regs = conf["regs"]
        self.is_pairwise = conf["is_pairwise"]
        self.topK = conf["topk"]
        self.lambda_bilinear = self.regs[0]
        self.gamma_bilinear = self.regs[1]
        self.eta_bilinear = self.regs[2]
        self.alpha = conf["alpha"]
        self.beta = conf["beta"]
        self.num_negatives = conf["num_neg"]
        self.learning_rate = conf["learning_rate"]
        self.activation = conf["activation"]
        self.loss_function = conf["loss_function"]
        self.algorithm = conf["algorithm"]
        self.learner = conf["learner"]
        self.embed_init_method = conf["embed_init_method"]
        self.weight_init_method = conf["weight_init_method"]
        self.stddev = conf["stddev"]
        self.pretrain_file = conf["pretrain_file"]
        # not keys of the reference
        self.attention_mask = conf["attention_mask"] if "attention_mask" in conf else "reference"
        self.c1_application = conf["c1_application"] if "c1_application" in conf else "dense"
        self.dataset = dataset
        self.num_items = dataset.num_items
        self.num_users = dataset.num_users
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...nais import ACTIVATIONS, MAX_D, MAX_W, NAISEngine, activation_code
        require_single_gpu("NAIS")
        d, w = self.embedding_size, self.weight_size
        if d < 1 or d > MAX_D:
            raise NotImplementedError("NAIS: embedding_size=%d is not supported (1 to %d)" % (d, MAX_D))
        if w < 1 or w > MAX_W:
            raise NotImplementedError("NAIS: weight_size=%d is not supported (1 to %d)" % (w, MAX_W))
        if not float(self.beta) >= 0.0:
            raise ValueError("NAIS needs beta >= 0, got %r" % (self.beta,))
        # NAIS.py:136-145: self.mlp_pretrain does not exist, so the try block always fails; nothing is loaded
        self.logger.info("load pretrained params unsuccessful!")
        self.logger.info("activation: %s" % ACTIVATIONS.get(activation_code(self.activation),
                                                            "none (activation=%r is not 0, 1 or 2)" % (self.activation,)))
        self.logger.info("attention mask: %s" % ("reference (num_idx = |H| + 1: one padding row for histories shorter "
                                                 "than the batch side's longest)" if self.attention_mask == "reference"
                                                 else "history (the softmax over the history alone)"))
        embed_init = get_initializer(self.embed_init_method, self.stddev, seed=2017)
        c1 = embed_init([self.num_items, d])
        Q = embed_init([self.num_items, d])
        weight_init = get_initializer(self.weight_init_method, self.stddev, seed=2017)
        W = weight_init([(self.algorithm + 1) * d, w])
        b = weight_init([1, w])
        self.engine = NAISEngine(c1, Q, W, b, self.dataset.train_matrix, self.learning_rate, self.regs, self.alpha,
                                 self.beta, self.batch_size, algorithm=self.algorithm, activation=self.activation,
                                 loss=self.loss_function, pairwise=self.is_pairwise is True, learner=self.learner,
                                 attention_mask=self.attention_mask, c1_application=self.c1_application)

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
