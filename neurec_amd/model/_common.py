"""Shared host code of the HIP-backed recommenders, general and sequential."""
from time import time

import numpy as np

PAIRWISE_STRUCTURE = "pairwise structure: positive side = history without the item (n = |R_u|), negative side = " \
                     "whole history (n = |R_u| + 1), users with one train item skipped"
POINTWISE_STRUCTURE = "pointwise structure: label 1 = history without the item (n = |R_u|), label 0 = whole history " \
                      "(n = |R_u| + 1)"


def require_single_gpu(name):
    """the refusal of a model whose engine has no multi-rank form"""
    from .. import parallel
    if parallel.get_comm().active:
        raise NotImplementedError("%s runs on one GPU: a multi-rank run (WORLD_SIZE > 1) is not supported; "
                                  "start it as a single process" % name)


def last_item_of(train_dict, num_users):
    """int32 [U]: the user's last train item by time, -1 for a user without train items"""
    last = np.full(num_users, -1, dtype=np.int32)
    for user, items in train_dict.items():
        if len(items):
            last[user] = items[-1]
    return last


def last_items_table(train_dict, num_users, high_order):
    """int32 [U, L]: the user's last min(L, |R_u|) train items ascending in time from column 0, -1 in the remaining
    columns and in the rows of users without train items — what predict() of Fossil pairs with eta columns 0..L-1 and
    the attention of FPMCplus runs over (the softmax covers the items there are)"""
    L = int(high_order)
    last = np.full((int(num_users), L), -1, dtype=np.int32)
    for user, items in train_dict.items():
        tail = list(items)[-L:]
        last[int(user), :len(tail)] = tail
    return last


def predict_scores(user_table, item_table, user_ids, candidate_items=None):
    """`predict` contract of the reference models (MF.py:120-134): a [B, I] float32 array, or
    — in candidate mode — a list of per-user score arrays.  The scores are computed by the
    fp32-MFMA scoring kernel and copied to the host (this entrance exists for plugin
    compatibility; the evaluator itself uses the on-device factor path)."""
    import torch
    from .. import engine as E
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
    from ..data import PairwiseSampler, PointwiseSampler
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


def train_time_order_model(model, high_order, pairwise, note, log_loss=True, step=None):
    """train_model of the sequential models that draw from the time-order samplers (FPMC.py:104-133 and its kin) on
    model.engine: the device instance streams at `high_order`, one loss copy per epoch, the reference's log lines
    (`note`: the model's deviations, logged once).  step(users, recent, items, third, loss_out): what runs per batch
    when the sampler's `recent` field needs reshaping before engine.step (None: engine.step itself).  The epochs'
    loss figures are kept in model.epoch_losses; log_loss=False: they are not logged."""
    import torch
    from .. import engine as E
    from ..data import TimeOrderPairwiseSampler, TimeOrderPointwiseSampler
    if step is None:
        step = model.engine.step
    model.logger.info(model.evaluator.metrics_info())
    model.logger.info(note)
    if pairwise:
        data_iter = TimeOrderPairwiseSampler(model.dataset, high_order=high_order, neg_num=1,
                                             batch_size=model.batch_size, shuffle=True, as_tensors=True)
    else:
        data_iter = TimeOrderPointwiseSampler(model.dataset, high_order=high_order, neg_num=model.num_negatives,
                                              batch_size=model.batch_size, shuffle=True, as_tensors=True)
    losses = torch.zeros((max(len(data_iter), 1), 2), device=E.require_gpu())
    model.epoch_losses = []
    for epoch in range(1, model.num_epochs + 1):
        num_training_instances = len(data_iter)           # the number of BATCHES, as the reference has it
        training_start_time = time()
        n = 0
        for bat_users, bat_items_recent, bat_items, bat_third in data_iter:
            step(bat_users, bat_items_recent, bat_items, bat_third, losses[n])
            n += 1
        per_step = losses[:n].cpu().numpy()               # one D2H copy per epoch
        total_loss = 0.0
        for a, b in per_step:                              # `total_loss += loss`
            total_loss += np.float32(a) + np.float32(b)
        model.epoch_losses.append(total_loss / max(num_training_instances, 1))
        if log_loss:
            model.logger.info("[iter %d : loss : %f, time: %f]" % (epoch, model.epoch_losses[-1],
                                                                   time() - training_start_time))
        if epoch % model.verbose == 0:
            model.logger.info("epoch %d:\t%s" % (epoch, model.evaluate()))
