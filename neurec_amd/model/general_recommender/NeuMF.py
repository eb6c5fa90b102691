"""NeuMF on the HIP engine.

Reference: Xiangnan He et al., "Neural Collaborative Filtering." in WWW 2017.
Plugin-compatible with model/general_recommender/NeuMF.py: same constructor, config keys (conf/NeuMF.properties: epochs,
batch_size, embedding_size, layers, reg_mf, reg_mlp, is_pairwise, num_neg, loss_function, learning_rate, learner,
init_method, stddev, verbose, mf_pretrain, mlp_pretrain), log lines and `predict` contract.  The per-batch
`sess.run((loss, optimizer))` and the per-user `sess.run` of predict() are neurec_amd/neumf.py (csrc/neumf.hip).

As the reference: the score is sum(p_u * q_i) + sum(h_last) with no learned output layer and no sigmoid; the first
layer reads 2 * int(layers[0] / 2) values, which is layers[0] only when that is even; the regulariser is taken on the
gathered rows; `mf_pretrain` and `mlp_pretrain` are unpickled as [user_table, item_table] each and used only when both
load ("load pretrained params successful!" / "... unsuccessful!"); the dense layers are always fresh; one sampler is made
before the first epoch.

Deviations, on purpose:
  * `is_pairwise=True` is refused.  NeuMF.py calls `tf.layers.dense` inside `_create_inference`, so its pairwise graph
    builds a SECOND, unshared layer stack for the negative item, whose weights never reach predict().  Sharing the stack
    would be a different model with no reference trace to hold it to; pairwise mode is left for a later change.
  * the instances come from the device `PointwiseSampler` stream, the initial values from numpy generators seeded 2017
    (embeddings by `init_method`, then the kernels glorot-uniform, biases zero, in the reference's creation order);
  * multi-rank runs are refused; predict() in full mode returns the [B, num_items] device tensor of
    `NeuMFEngine.score`, in candidate mode per-user numpy arrays from `NeuMFEngine.forward`.
"""
import pickle
from time import time

import numpy as np

from ...util import timer
from ...util.tool import get_initializer
from ..AbstractRecommender import AbstractRecommender
from .._common import require_single_gpu

PAIRWISE_REFUSAL = ("NeuMF: is_pairwise=True is not supported: the reference's pairwise graph gives the negative item a "
                    "second, unshared layer stack (tf.layers.dense inside _create_inference) whose weights never reach "
                    "predict(); run with is_pairwise=False and a pointwise loss_function (cross_entropy, square)")


def load_pretrained(mf_pretrain, mlp_pretrain):
    """[[mf_user, mf_item], [mlp_user, mlp_item]] as build_graph of NeuMF.py:108-117 reads them, None on any exception"""
    try:
        params = []
        with open(mf_pretrain, "rb") as fin:
            params.append(pickle.load(fin, encoding="utf-8"))
        with open(mlp_pretrain, "rb") as fin:
            params.append(pickle.load(fin, encoding="utf-8"))
        return [[np.asarray(t, dtype=np.float32) for t in (p[0], p[1])] for p in params]
    except Exception:
        return None


def initial_variables(num_users, num_items, embedding_size, layers, init_method, stddev, params=None, with_mf=True):
    """{name: array} in the reference's creation order: the embeddings from `init_method` (or `params`), then per layer
    a glorot-uniform kernel and a zero bias"""
    from ...neumf import layer_inputs
    init = get_initializer(init_method, stddev, seed=2017)
    e = int(layers[0] / 2)
    out = {}
    if with_mf:
        out["mf_embedding_user"] = params[0][0] if params else init([num_users, embedding_size])
        out["mf_embedding_item"] = params[0][1] if params else init([num_items, embedding_size])
    out["mlp_embedding_user"] = params[1][0] if params else init([num_users, e])
    out["mlp_embedding_item"] = params[1][1] if params else init([num_items, e])
    glorot = get_initializer("xavier_uniform", stddev, seed=2017)
    for k, (n_in, w) in enumerate(zip(layer_inputs(layers), layers)):
        out["kernel%d" % k] = np.asarray(glorot([n_in, int(w)]), dtype=np.float32).reshape(n_in, int(w))
        out["bias%d" % k] = np.zeros(int(w), dtype=np.float32)
    return out


def train_pointwise_model(model, sampler_per_epoch):
    """train_model of NeuMF.py:123-151 / MLP.py:95-124 on model.engine: the device PointwiseSampler stream, one loss
    copy per epoch, the reference's log lines.  sampler_per_epoch: MLP.py builds a fresh sampler in every epoch"""
    import torch
    from ...data import PointwiseSampler
    engine = model.engine
    model.logger.info(model.evaluator.metrics_info())

    def sampler(epoch):
        return PointwiseSampler(model.dataset, neg_num=model.num_negatives, batch_size=model.batch_size, shuffle=True,
                                drop_last=False, as_tensors=True, seed=2018 + epoch)
    data_iter = sampler(0)
    losses = torch.zeros((max(len(data_iter), 1), 2), device=engine.T["mlp_embedding_user"].device)
    for epoch in range(1, model.num_epochs + 1):
        if sampler_per_epoch and epoch > 1:
            data_iter = sampler(epoch - 1)
        training_start_time = time()
        num_training_instances = len(data_iter)           # the number of BATCHES, as the reference has it
        n = 0
        for bat_users, bat_items, bat_labels in data_iter:
            engine.step(bat_users, bat_items, bat_labels, losses[n])
            n += 1
        per_step = losses[:n].cpu().numpy()               # one D2H copy per epoch
        total_loss = 0.0
        for a, b in per_step:                              # `total_loss += loss`
            total_loss += np.float32(a) + np.float32(b)
        model.logger.info("[iter %d : loss : %f, time: %f]" % (epoch, total_loss / max(num_training_instances, 1),
                                                               time() - training_start_time))
        if epoch % model.verbose == 0:
            model.logger.info("epoch %d:\t%s" % (epoch, model.evaluate()))


def predict_pairs(engine, user_ids, candidate_items_userids):
    """full mode: the device tensor; candidate mode: per-user numpy arrays of the candidates' scores"""
    users = np.asarray(list(user_ids), dtype=np.int32)
    if candidate_items_userids is None:
        return engine.score(users)
    sizes = [len(items) for items in candidate_items_userids]
    flat_items = np.concatenate([np.asarray(items, dtype=np.int32).reshape(-1) for items in candidate_items_userids]) \
        if sizes else np.zeros(0, np.int32)
    flat = engine.forward(np.repeat(users, sizes).astype(np.int32), flat_items).cpu().numpy()
    return np.split(flat, np.cumsum(sizes)[:-1]) if sizes else []


class NeuMF(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(NeuMF, self).__init__(dataset, conf)
        self.embedding_size = conf["embedding_size"]
        self.layers = conf["layers"]
        self.reg_mf = conf["reg_mf"]
        self.reg_mlp = conf["reg_mlp"]
        self.learning_rate = conf["learning_rate"]
        self.learner = conf["learner"]
        self.loss_function = conf["loss_function"]
        self.num_epochs = conf["epochs"]
        self.num_negatives = conf["num_neg"]
        self.batch_size = conf["batch_size"]
        self.verbose = conf["verbose"]
        self.is_pairwise = conf["is_pairwise"]
        self.mf_pretrain = conf["mf_pretrain"]
        self.mlp_pretrain = conf["mlp_pretrain"]
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.dataset = dataset
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...neumf import MAX_WIDTH, NeuMFEngine, check_shape
        require_single_gpu("NeuMF")
        if self.is_pairwise is True:
            raise NotImplementedError(PAIRWISE_REFUSAL)
        layers = check_shape("NeuMF", self.embedding_size, self.layers)
        if int(self.embedding_size) < 1:
            raise NotImplementedError("NeuMF: embedding_size=%d is not supported (1 to %d)" % (self.embedding_size,
                                                                                              MAX_WIDTH))
        params = load_pretrained(self.mf_pretrain, self.mlp_pretrain)
        self.logger.info("load pretrained params successful!" if params is not None
                         else "load pretrained params unsuccessful!")
        d = int(self.embedding_size) if params is None else int(params[0][0].shape[1])
        variables = initial_variables(self.num_users, self.num_items, d, layers, self.init_method, self.stddev, params)
        self.engine = NeuMFEngine(variables, layers, self.learning_rate, self.reg_mf, self.reg_mlp, self.batch_size,
                                  loss=self.loss_function, learner=self.learner, name="NeuMF")

    def train_model(self):
        train_pointwise_model(self, sampler_per_epoch=False)

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def predict(self, user_ids, candidate_items_user_ids=None):
        """Full mode: the [B, num_items] score rows as a device tensor (the evaluator's score-matrix path reads it in
        place).  Candidate mode: a list of per-user numpy arrays."""
        return predict_pairs(self.engine, user_ids, candidate_items_user_ids)
