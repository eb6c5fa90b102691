"""ConvNCF on the HIP engine.

Reference: Xiangnan He et al., "Outer Product-based Neural Collaborative Filtering", In IJCAI 2018.
Plugin-compatible with model/general_recommender/ConvNCF.py: same constructor, config keys (conf/ConvNCF.properties:
epochs, batch_size, embedding_size, regs, net_channel, lr_embed, lr_net, num_negatives, loss_function, keep,
embed_init_method, weight_init_method, stddev, verbose), log lines and `predict` contract.  The per-batch
`sess.run((self.loss, self.optimizer))` and the per-user `sess.run` of predict() are neurec_amd/convncf.py
(csrc/convncf.hip).

As the reference: the score is the conv tower's last activation times W plus b, with no sigmoid; the conv biases start at
0.1; the embedding regulariser regs[0] is taken on the gathered rows p1, q2, q1 (the user row once per triplet — the
second inference's p2 is never counted); regs[1] weighs l2(W, b) and regs[2] weighs the conv kernels and biases and
l2(W, b) once more; the logged loss is `self.loss`, without the regularisers, summed over a batch and divided by the
number of BATCHES; the learner is two plain tf.train.AdagradOptimizer (lr_embed for the tables, lr_net for the rest) whose
accumulators start at 0.1; `keep` is read and never fed, so dropout is never on; `num_negatives` is read but the sampler
is PairwiseSampler(neg_num=1); build_graph reads `self.mf_pretrain`, which does not exist, so it always logs "load
pretrained params unsuccessful!" and starts fresh; the pre-optimiser that the reference builds is never run and is not
built here.

Deviations, on purpose:
  * the graph means one value per pair only when embedding_size == 2**len(net_channel) (otherwise the reference's
    reshape yields several rows per pair and predict() more than one value per item): every other shape is refused, as
    are more than 6 layers and more than 32 channels;
  * the triplets come from the device `PairwiseSampler` stream, drawn once before the first epoch, the initial values
    from numpy generators seeded 2017 in the reference's creation order (a conv kernel's fans are TF's: 4 c_in, 4 c_out);
  * multi-rank runs are refused; predict() in full mode returns the [B, num_items] device tensor of
    `ConvNCFEngine.score`, in candidate mode per-user numpy arrays from `ConvNCFEngine.forward`.
"""
from time import time

import numpy as np

from ...util import timer
from ...util.tool import get_initializer
from ..AbstractRecommender import AbstractRecommender
from .._common import require_single_gpu
from .NeuMF import predict_pairs


def weight_initializer(method, stddev, shape, seed):
    """`weight_init_method` on `shape` with TF's fans: for a conv kernel [h, w, c_in, c_out] they are h w c_in and
    h w c_out; util.tool.get_initializer reads the first two entries of a shape, which is right for matrices only"""
    shape = tuple(int(n) for n in shape)
    field = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    fi, fo = (shape[-2] * field, shape[-1] * field) if len(shape) >= 2 else (shape[0], shape[0])
    spread = {"xavier_normal": ("tnormal", np.sqrt(1.3 * 2.0 / (fi + fo))),
              "xavier_uniform": ("uniform", np.sqrt(6.0 / (fi + fo))),
              "he_normal": ("tnormal", np.sqrt(1.3 * 2.0 / fi)),
              "he_uniform": ("uniform", np.sqrt(6.0 / fi))}
    kind, width = spread.get(method, (method, stddev))
    return get_initializer(kind, width, seed=seed)(shape)


def initial_variables(num_users, num_items, embedding_size, net_channel, embed_init_method, weight_init_method, stddev):
    """{name: array} in the reference's creation order (ConvNCF.py:64-85): the tables from `embed_init_method`, per
    layer a kernel from `weight_init_method` and a bias of 0.1, then W and b from `weight_init_method`"""
    init = get_initializer(embed_init_method, stddev, seed=2017)
    out = {"embedding_P": init([num_users, embedding_size]), "embedding_Q": init([num_items, embedding_size])}
    c_in = 1
    for k, c in enumerate(net_channel):
        out["kernel%d" % k] = weight_initializer(weight_init_method, stddev, [2, 2, c_in, int(c)], 2018 + k)
        out["bias%d" % k] = np.full(int(c), 0.1, dtype=np.float32)
        c_in = int(c)
    out["W"] = weight_initializer(weight_init_method, stddev, [c_in, 1], 2018 + len(net_channel))
    out["b"] = weight_initializer(weight_init_method, stddev, [1], 2019 + len(net_channel))
    return out


class ConvNCF(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(ConvNCF, self).__init__(dataset, conf)
        self.embedding_size = conf["embedding_size"]
        regs = conf["regs"]
        self.lambda_bilinear = regs[0]
        self.gamma_bilinear = regs[1]
        self.lambda_weight = regs[2]
        self.keep = conf["keep"]              # read, never fed: the reference's dropout is never on
        self.num_epochs = conf["epochs"]
        self.batch_size = conf["batch_size"]
        self.nc = conf["net_channel"]
        self.lr_embed = conf["lr_embed"]
        self.lr_net = conf["lr_net"]
        self.verbose = conf["verbose"]
        self.loss_function = conf["loss_function"]
        self.num_negatives = conf["num_negatives"]   # read; the sampler draws one negative
        self.embed_init_method = conf["embed_init_method"]
        self.weight_init_method = conf["weight_init_method"]
        self.stddev = conf["stddev"]
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.dataset = dataset
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...convncf import ConvNCFEngine, check_shape
        require_single_gpu("ConvNCF")
        channels = check_shape(self.embedding_size, self.nc)
        self.logger.info("load pretrained params unsuccessful!")     # ConvNCF.py:149-158: self.mf_pretrain does not exist
        variables = initial_variables(self.num_users, self.num_items, int(self.embedding_size), channels,
                                      self.embed_init_method, self.weight_init_method, self.stddev)
        self.engine = ConvNCFEngine(variables, channels, self.lr_embed, self.lr_net,
                                    [self.lambda_bilinear, self.gamma_bilinear, self.lambda_weight], self.batch_size,
                                    loss=self.loss_function)

    def train_model(self):
        import torch
        from ...data import PairwiseSampler
        engine = self.engine
        self.logger.info(self.evaluator.metrics_info())
        data_iter = PairwiseSampler(self.dataset, neg_num=1, batch_size=self.batch_size, shuffle=True, as_tensors=True)
        losses = torch.zeros((max(len(data_iter), 1), 2), device=engine.T["embedding_P"].device)
        for epoch in range(1, self.num_epochs + 1):
            total_loss = 0.0
            training_start_time = time()
            num_training_instances = len(data_iter)           # the number of BATCHES, as the reference has it
            n = 0
            for bat_users, bat_items_pos, bat_items_neg in data_iter:
                engine.step(bat_users, bat_items_pos, bat_items_neg, losses[n])
                n += 1
            for loss in losses[:n, 0].cpu().numpy():          # one D2H copy per epoch; `total_loss += loss`
                total_loss += loss
            self.logger.info("[iter %d : loss : %f, time: %f]" % (epoch, total_loss / max(num_training_instances, 1),
                                                                  time() - training_start_time))
            if epoch % self.verbose == 0:
                self.logger.info("epoch %d:\t%s" % (epoch, self.evaluate()))

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def predict(self, user_ids, candidate_items_user_ids=None):
        """Full mode: the [B, num_items] output rows as a device tensor (the evaluator's score-matrix path reads it in
        place).  Candidate mode: a list of per-user numpy arrays."""
        return predict_pairs(self.engine, user_ids, candidate_items_user_ids)
