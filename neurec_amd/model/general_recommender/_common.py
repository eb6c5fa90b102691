"""Shared host code of the HIP-backed general recommenders."""
from time import time

import numpy as np

PAIRWISE_STRUCTURE = "pairwise structure: positive side = history without the item (n = |R_u|), negative side = " \
                     "whole history (n = |R_u| + 1), users with one train item skipped"
POINTWISE_STRUCTURE = "pointwise structure: label 1 = history without the item (n = |R_u|), label 0 = whole history " \
                      "(n = |R_u| + 1)"


def predict_scores(user_table, item_table, user_ids, candidate_items=None):
    """`predict` contract of the reference models (MF.py:120-134): a [B, I] float32 array, or
    — in candidate mode — a list of per-user score arrays.  The scores are computed by the
    fp32-MFMA scoring kernel and copied to the host (this entrance exists for plugin
    compatibility; the evaluator itself uses the on-device factor path)."""
    import torch
    from ... import engine as E
    users = torch.tensor(np.asarray(list(user_ids), dtype=np.int32), device=user_table.device)
    gemm = E.score_gemm_for(item_table, max(users.numel(), 1))
    ratings = gemm(user_table, users).cpu().numpy()[:, :item_table.shape[0]]
    if candidate_items is not None:
        return [rating[items] for rating, items in zip(ratings, candidate_items)]
    return np.ascontiguousarray(ratings)


def train_history_model(model, before_batches=None, after_epoch=None):
    """train_model of the history models (FISM.py:118-142, NAIS.py:196-220) on model.engine: the device instance
    streams instead of the reference's numpy generator, one loss copy per epoch, the reference's log lines.
    before_batches(batches) -> further keyword arguments of engine.step for the epoch (the epoch's batches are then
    drawn ahead as a list); after_epoch(): called once the epoch's losses are on the host."""
    import torch
    from ...data import PairwiseSampler, PointwiseSampler
    engine = model.engine
    model.logger.info(model.evaluator.metrics_info())
    pairwise = model.is_pairwise is True
    model.logger.info(PAIRWISE_STRUCTURE if pairwise else POINTWISE_STRUCTURE)
    if pairwise:
        data_iter = PairwiseSampler(model.dataset, neg_num=1, batch_size=model.batch_size, shuffle=True,
                                    as_tensors=True)
        deg = engine.h_deg
        n_instances = int(deg[deg > 1].sum())              # data_generator.py:13: users with more than one item
    else:
        data_iter = PointwiseSampler(model.dataset, neg_num=model.num_negatives, batch_size=model.batch_size,
                                     shuffle=True, as_tensors=True)
        n_instances = engine.csr.nnz * (1 + model.num_negatives)
    losses = torch.zeros((max(len(data_iter), 1), 2), device=engine.c1.device)
    for epoch in range(1, model.num_epochs + 1):
        training_start_time = time()
        n = 0
        batches, more = data_iter, {}
        if before_batches is not None:
            batches = list(data_iter)
            more = before_batches(batches)
        for bat_users, bat_items, bat_third in batches:
            engine.step(bat_users, bat_items, bat_third, losses[n], **more)
            n += 1
        per_step = losses[:n].cpu().numpy()               # one D2H copy per epoch
        if after_epoch is not None:
            after_epoch()
        total_loss = 0.0
        for a, b in per_step:                              # `total_loss += loss`, FISM.py:130,139
            total_loss += np.float32(a) + np.float32(b)
        model.logger.info("[iter %d : loss : %f, time: %f]" % (epoch, total_loss / max(n_instances, 1),
                                                               time() - training_start_time))
        if epoch % model.verbose == 0:
            model.logger.info("epoch %d:\t%s" % (epoch, model.evaluate()))
