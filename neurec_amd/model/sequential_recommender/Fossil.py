"""Fossil on the HIP engine.

Reference: Ruining He et al., "Fusing similarity models with Markov chains for sparse sequential recommendation." ICDM
2016.  Plugin-compatible with model/sequential_recommender/Fossil.py: same constructor, config keys
(conf/Fossil.properties: epochs, batch_size, embedding_size, regs (three entries), alpha, learning_rate, learner,
is_pairwise, high_order, num_neg, loss_function, init_method, stddev, verbose), log lines and `predict` contract.  The
per-batch `sess.run((loss, optimizer))` on histories padded to [B, Lmax] is neurec_amd/fossil.py (csrc/fossil.hip); the
instances come from the device streams of the time-order samplers at high_order = L.

Deviations, on purpose:
1. The reference's generators (_get_*_all_likefossil_data) append one aliased list per user and then mutate it, so the
   histories its graph sees are not the ones the code spells out.  Here the structure the generator states: positive /
   label 1 = the history without the item, n = |R_u| - 1; negative / label 0 = the whole history, n = |R_u|; users with
   |R_u| <= L take no part.  The recents of the instance at sequence position idx are seq[idx-1], ..., seq[idx-L], most
   recent first (the samplers deliver them ascending: `recents_for_engine` reverses them).
2. predict() pairs eta column 0 with the OLDEST of the last L items (the reference feeds seq[len-L:] ascending), while
   training pairs it with the most recent.  Kept: it is what the reference scores.
3. A user with |R_u| < L is scored on its last |R_u| items, ascending, at eta columns 0.., the remaining columns meet
   the zero row (the reference's slice gives a ragged feed); a user without train items scores `bias` alone.  Candidate
   mode returns the candidates' entries of the full-mode rows.
"""
from time import time

import numpy as np

from ...util import timer
from ...util.tool import get_initializer
from ..AbstractRecommender import SeqAbstractRecommender
from .._common import last_items_table, predict_scores, require_single_gpu

STRUCTURE = "instance structure: positive / label 1 = history without the item (n = |R_u| - 1), negative / label 0 = " \
            "whole history (n = |R_u|), users with |R_u| <= high_order skipped; recents most recent first in " \
            "training, predict() pairs eta column 0 with the oldest of the last high_order items; users with fewer " \
            "train items are scored on those alone, users without any on the bias"


def recents_for_engine(recent, high_order):
    """The samplers' `recent` field (seq[idx-L..idx-1] ascending; [B] when L = 1) as the engine takes it: [B, L] with
    column l = seq[idx-1-l].  numpy arrays and torch tensors alike."""
    recent = recent.reshape(-1, high_order)
    if high_order == 1:
        return recent
    if isinstance(recent, np.ndarray):
        return np.ascontiguousarray(recent[:, ::-1])
    return recent.flip(1).contiguous()


class Fossil(SeqAbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(Fossil, self).__init__(dataset, conf)
        self.verbose = conf["verbose"]
        self.batch_size = conf["batch_size"]
        self.num_epochs = conf["epochs"]
        self.embedding_size = conf["embedding_size"]
        regs = conf["regs"]
        self.regs = regs
        self.lambda_bilinear = regs[0]
        self.gamma_bilinear = regs[1]
        self.reg_eta = regs[2]
        self.alpha = conf["alpha"]
        self.num_negatives = conf["num_neg"]
        self.learning_rate = conf["learning_rate"]
        self.learner = conf["learner"]
        self.loss_function = conf["loss_function"]
        self.is_pairwise = conf["is_pairwise"]
        self.high_order = conf["high_order"]
        self.init_method = conf["init_method"]
        self.stddev = conf["stddev"]
        self.num_users = dataset.num_users
        self.num_items = dataset.num_items
        self.dataset = dataset
        self.train_matrix = self.dataset.train_matrix
        self.train_dict = dataset.get_user_train_dict(by_time=True)
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None
        self.last_items = None

    def build_graph(self):
        from ...fossil import FossilEngine
        require_single_gpu("Fossil")
        init = get_initializer(self.init_method, self.stddev, seed=2017)   # main.py:12
        c1 = init([self.num_items, self.embedding_size])                   # creation order of Fossil.py:63-70
        Q = init([self.num_items, self.embedding_size])
        eta = init([self.num_users, self.high_order])
        eta_bias = init([1, self.high_order])
        last = last_items_table(self.train_dict, self.num_users, self.high_order)
        self.engine = FossilEngine(c1, Q, eta, eta_bias, self.train_matrix, self.learning_rate, self.regs, self.alpha,
                                   self.batch_size, loss=self.loss_function, pairwise=self.is_pairwise is True,
                                   learner=self.learner, last_items=last)
        self.last_items = self.engine.last_items

    # ---------- training process -------
    def train_model(self):
        import torch
        from ...data import TimeOrderPairwiseSampler, TimeOrderPointwiseSampler
        engine, L = self.engine, self.high_order
        self.logger.info(self.evaluator.metrics_info())
        self.logger.info(STRUCTURE)
        if self.is_pairwise is True:
            data_iter = TimeOrderPairwiseSampler(self.dataset, high_order=L, neg_num=1, batch_size=self.batch_size,
                                                 shuffle=True, as_tensors=True)
        else:
            data_iter = TimeOrderPointwiseSampler(self.dataset, high_order=L, neg_num=self.num_negatives,
                                                  batch_size=self.batch_size, shuffle=True, as_tensors=True)
        # Fossil.py:134: len(user_input) — the pairs, or the windows x (1 + num_neg)
        num_training_instances = data_iter.stream.n_slots
        losses = torch.zeros((max(len(data_iter), 1), 2), device=engine.c1.device)
        for epoch in range(1, self.num_epochs + 1):
            training_start_time = time()
            n = 0
            for bat_users, bat_items_recent, bat_items, bat_third in data_iter:
                engine.step(bat_users, recents_for_engine(bat_items_recent, L), bat_items, bat_third, losses[n])
                n += 1
            per_step = losses[:n].cpu().numpy()           # one D2H copy per epoch
            total_loss = 0.0
            for a, b in per_step:                          # `total_loss += loss`, Fossil.py:153,165
                total_loss += np.float32(a) + np.float32(b)
            self.logger.info("[iter %d : loss : %f, time: %f]" %
                             (epoch, total_loss / max(num_training_instances, 1), time() - training_start_time))
            if epoch % self.verbose == 0:
                self.logger.info("epoch %d:\t%s" % (epoch, self.evaluate()))

    @timer
    def evaluate(self):
        return self.evaluator.evaluate(self)

    def get_eval_factors(self):
        """Device tables for the evaluator's on-GPU factor path: [ |R_u|^-alpha p_u + s_u | 1 ] against [Q | bias]."""
        return self.engine.eval_factors(self.last_items)

    def predict(self, user_ids, candidate_items_userids=None):
        P, Q = self.engine.eval_factors(self.last_items)
        return predict_scores(P, Q, user_ids, candidate_items_userids)
