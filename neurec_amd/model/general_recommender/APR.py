"""APR on the HIP engine.

Reference: Xiangnan He et al., "Adversarial Personalized Ranking for Recommendation." SIGIR 2018.
Plugin-compatible with model/general_recommender/APR.py: same constructor, config keys (conf/APR.properties),
epoch loop, log lines and `predict` contract; a step is one native call (neurec_amd/apr.py, csrc/apr.hip) plus the
optimiser's application on tables that never leave HBM.

Kept and deviating:
  * The reference class builds the adversarial graph (APR.py:83-118) and never runs it: `_create_optimizer` minimises
    `self.loss` (APR.py:122), `train_model` never fetches `update_P` / `update_Q` (APR.py:132-150) and `adv_epoch` is
    read (APR.py:25) and used nowhere — as shipped it is BPR-MF with a summed softplus loss, and reg, reg_adv, eps,
    adv, adver and adv_epoch have no effect.  By default this plugin RUNS the graph the class builds, the way the paper
    and the comments of conf/APR.properties describe it: epoch e (1-based) is adversarial when `adver` is truthy and
    e > adv_epoch; a step of such an epoch sets Delta from the current tables and its batch (adv=grad) or from a fresh
    draw (adv=random), then minimises opt_loss; any other epoch minimises loss + reg * l2 (the adver = 0 graph).
    `--reference_train_loop=True` reproduces the loop as shipped: every step minimises `loss` alone.
  * The logged loss is `self.loss` in every mode: the plain term at the incoming tables, summed over the steps and
    divided by the number of batches (APR.py:144-148).
  * Delta exists for the batch's rows only: a row outside the batch is never read in the step, so the reference's two
    dense assigns (APR.py:117-118) are not materialised.
  * Outside the shipped loop with reg == 0 the tables take the sparse application (the learners other than Adam move
    the batch's rows only); with reg != 0 the gradient is dense.
  * Under WORLD_SIZE > 1 every rank trains the whole model (same seeds, same tables).
"""
from time import time

import numpy as np

from ...data import PairwiseSampler
from ...util import timer
from ...util.tool import get_initializer
from ..AbstractRecommender import AbstractRecommender
from .._common import predict_scores


def _truthy(x):
    if isinstance(x, str):
        return x.strip().lower() not in ("", "0", "false", "none")
    return bool(x)


class APR(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(APR, self).__init__(dataset, conf)
        self.learning_rate = conf["learning_rate"]
        self.embedding_size = conf["embedding_size"]
        self.learner = conf["learner"]
        self.num_epochs = conf["epochs"]
        self.eps = conf["eps"]
        self.adv = conf["adv"]
        self.adver = conf["adver"]
        self.adv_epoch = conf["adv_epoch"]
        self.reg = conf["reg"]
        self.reg_adv = conf["reg_adv"]
        self.batch_size = conf["batch_size"]
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.verbose = conf["verbose"]
        self.dataset = dataset
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.sess = sess                      # unused: there is no TensorFlow session
        self.reference_train_loop = _truthy(conf["reference_train_loop"]) if "reference_train_loop" in conf else False
        if self.reference_train_loop:
            self.logger.info("reference_train_loop=True: every step minimises `loss` alone, as APR.py:122 builds the "
                             "optimizer and APR.py:132-150 runs it (update_P / update_Q are never fetched, adv_epoch "
                             "of APR.py:25 is unused): reg, reg_adv, eps, adv, adver and adv_epoch have no effect")
        else:
            self.logger.info("reference_train_loop=False (default): the adversarial graph of APR.py:83-118 is run — "
                             "epochs after adv_epoch=%s perturb (adver=%s, adv=%s) and minimise opt_loss; the reference "
                             "minimises `loss` alone (APR.py:122, 132-150) — pass --reference_train_loop=True to "
                             "reproduce it" % (self.adv_epoch, self.adver, self.adv))
        self.engine = None

    def build_graph(self):
        from ...apr import APREngine
        init = get_initializer(self.init_method, self.stddev, seed=2017)   # main.py:12
        users = init([self.num_users, self.embedding_size])
        items = init([self.num_items, self.embedding_size])
        self.engine = APREngine(users, items, self.learning_rate, self.reg, self.reg_adv, self.eps, self.batch_size,
                                adv=self.adv, learner=self.learner)

    def is_adversarial(self, epoch):
        from ...apr import adversarial_epoch
        return adversarial_epoch(epoch, _truthy(self.adver), self.adv_epoch, self.reference_train_loop)

    # ---------- training process -------
    def train_model(self):
        import torch
        self.logger.info(self.evaluator.metrics_info())
        data_iter = PairwiseSampler(self.dataset, neg_num=1, batch_size=self.batch_size, shuffle=True, as_tensors=True)
        losses = torch.zeros((max(len(data_iter), 1), 2), device=self.engine.P.device)
        for epoch in range(1, self.num_epochs + 1):
            training_start_time = time()
            num_training_instances = len(data_iter)
            adversarial, with_reg = self.is_adversarial(epoch), not self.reference_train_loop
            n = 0
            for bat_users, bat_items_pos, bat_items_neg in data_iter:
                self.engine.step(bat_users, bat_items_pos, bat_items_neg, losses[n], adversarial=adversarial,
                                 with_reg=with_reg)
                n += 1
            per_step = losses[:n, 0].cpu().numpy()          # one D2H copy per epoch; `self.loss`, APR.py:144
            total_loss = 0.0
            for loss in per_step:                            # `total_loss += loss`, APR.py:145
                total_loss += np.float32(loss)
            self.logger.info("[iter %d : loss : %f, time: %f]" % (epoch, total_loss / num_training_instances,
                                                                 time() - training_start_time))
            if epoch % self.verbose == 0:
                self.logger.info("epoch %d:\t%s" % (epoch, self.evaluate()))

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def get_eval_factors(self):
        """Device tables for the evaluator's on-GPU factor path."""
        return self.engine.P, self.engine.Q

    def predict(self, user_ids, candidate_items=None):
        return predict_scores(self.engine.P, self.engine.Q, user_ids, candidate_items)
