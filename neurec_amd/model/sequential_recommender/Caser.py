"""Caser on the HIP engine.

Reference: Jiaxi Tang and Ke Wang, "Personalized Top-N Sequential Recommendation via Convolutional Sequence Embedding."
in WSDM 2018.
Plugin-compatible with model/sequential_recommender/Caser.py: same constructor, config keys (conf/Caser.properties: lr,
l2_reg, factors_num, seq_L, seq_T, nv, nh, dropout, neg_samples, batch_size, epochs), log lines and `predict` contract.
The per-step `sess.run(self.train_opt)` is neurec_amd/caser.py (csrc/caser.hip).

The sequences are the reference's (`_generate_sequences`, Caser.py:144-172): sliding windows of seq_L + seq_T items
from the end, or one front-padded row for a user with fewer items.  The feeds follow the reference's order on numpy's
global stream (Caser.py:129-131): `_sample_negative` first — the unique users in chunks of 1024,
`batch_randint_choice(I, count * neg_samples, replace=True, exclusion=train items)` reshaped to [count, neg_samples] —
then `DataIterator(shuffle=True)`'s permutation.  The initial values come from `get_initializer` with fixed seeds in the
creation order of the variables (glorot uniform, a conv kernel's fans counted over its receptive field as TF does;
item_biases and the layer biases zero); the dropout masks from the engine's counter-based device generator.

Deviations, on purpose:
  * a user with fewer than seq_T train items has the pad id I among its positives, which the reference looks up in a
    table of I rows: TF on a CPU raises there, TF on a GPU reads zeros.  Here such a target has logit 0 and no gradient
    and stays in the mean's denominator — the TF-on-GPU reading;
  * a user without train items scores concat(z of the all-padded row, its user row) (the reference raises KeyError);
  * a multi-rank run is refused by name.
"""
import numpy as np

from ...util import DataIterator, batch_randint_choice, pad_sequences
from ...util.tool import csr_to_user_dict_bytime, get_initializer
from .._common import require_single_gpu
from ..AbstractRecommender import SeqAbstractRecommender

DEVIATIONS = "a pad id among the positives (a user with fewer than seq_T train items) has logit 0 and no gradient, as " \
             "TF on a GPU reads it (TF on a CPU raises); users without train items score the all-padded row"


def generate_sequences(user_pos_train, items_num, seq_L, seq_T):
    """Caser._generate_sequences (Caser.py:144-172): (users_list, item_seq_list, item_pos_list, user_test_seq)"""
    user_test_seq = {}
    users_list, item_seq_list, item_pos_list = [], [], []
    seq_len = seq_L + seq_T
    for user in np.unique(list(user_pos_train.keys())):
        seq_items = user_pos_train[user]
        if len(seq_items) - seq_len >= 0:
            rows = [seq_items[i - seq_len:i] for i in range(len(seq_items), seq_len - 1, -1)]
        else:
            padded = pad_sequences(np.reshape(seq_items, [1, -1]).astype(np.int32), value=items_num, max_len=seq_len,
                                   padding="pre", truncating="pre")
            rows = [np.reshape(padded, [-1])]
        for seq_i in rows:
            if user not in user_test_seq:
                user_test_seq[user] = seq_i[-seq_L:]
            users_list.append(user)
            item_seq_list.append(seq_i[:seq_L])
            item_pos_list.append(seq_i[-seq_T:])
    return users_list, item_seq_list, item_pos_list, user_test_seq


def sample_negative(users_list, user_pos_train, items_num, neg_samples, sampler=batch_randint_choice):
    """Caser._sample_negative (Caser.py:174-189): one [neg_samples] row per entry of users_list"""
    neg_items_list, user_neg = [], {}
    all_uni_user, all_counts = np.unique(users_list, return_counts=True)
    for bat_users, bat_counts in DataIterator(all_uni_user, all_counts, batch_size=1024, shuffle=False):
        n_neg_items = [c * neg_samples for c in bat_counts]
        exclusion = [user_pos_train[u] for u in bat_users]
        bat_neg = sampler(items_num, n_neg_items, replace=True, exclusion=exclusion)
        for u, neg in zip(bat_users, bat_neg):
            user_neg[u] = neg
    for u, c in zip(all_uni_user, all_counts):
        neg_items_list.extend(np.reshape(user_neg[u], [c, neg_samples]))
    return neg_items_list


def epoch_feeds(users_list, item_seq_list, item_pos_list, user_pos_train, items_num, neg_samples, batch_size,
                sampler=batch_randint_choice):
    """The feeds of one epoch in the reference's numpy stream order: the negatives first, then the shuffle.  Returns
    users int32 [S, batch_size], seq [S, batch_size, seq_L], pos [S, batch_size, seq_T], neg [S, batch_size,
    neg_samples] — the last batch filled up (user 0, pad sequences and positives, negative 0) — and rows [S], the true
    size of each batch: the filling takes no part in a step."""
    neg_list = sample_negative(users_list, user_pos_train, items_num, neg_samples, sampler)
    n = len(users_list)
    arrays = [np.asarray(users_list, np.int32).reshape(n), np.asarray(item_seq_list, np.int32).reshape(n, -1),
              np.asarray(item_pos_list, np.int32).reshape(n, -1), np.asarray(neg_list, np.int32).reshape(n, neg_samples)]
    order = np.random.permutation(n) if n else np.zeros(0, np.int64)    # DataIterator(shuffle=True)
    S = (n + batch_size - 1) // batch_size
    fill = (0, items_num, items_num, 0)
    out = [np.full((S, batch_size) + a.shape[1:], v, np.int32) for a, v in zip(arrays, fill)]
    rows = np.zeros(S, np.int32)
    for s in range(S):
        idx = order[s * batch_size:(s + 1) * batch_size]
        rows[s] = len(idx)
        for o, a in zip(out, arrays):
            o[s, :len(idx)] = a[idx]
    return out[0], out[1], out[2], out[3], rows


class Caser(SeqAbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(Caser, self).__init__(dataset, conf)
        self.dataset = dataset
        self.users_num, self.items_num = dataset.train_matrix.shape
        self.lr = conf["lr"]
        self.l2_reg = conf["l2_reg"]
        self.factors_num = conf["factors_num"]
        self.batch_size = conf["batch_size"]
        self.epochs = conf["epochs"]
        self.seq_L = conf["seq_L"]
        self.seq_T = conf["seq_T"]
        self.nv = conf["nv"]
        self.nh = conf["nh"]
        self.dropout = conf["dropout"]
        self.neg_samples = conf["neg_samples"]
        self.user_pos_train = csr_to_user_dict_bytime(dataset.time_matrix, dataset.train_matrix)
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...caser import CaserEngine, table_names
        require_single_gpu("Caser")
        d, L, nv, nh = self.factors_num, self.seq_L, self.nv, self.nh
        embed = get_initializer("xavier_uniform", 0.01, seed=2017)      # get_variable's default: glorot uniform
        dense = get_initializer("xavier_uniform", 0.01, seed=2019)      # layers.Dense: glorot uniform

        def conv(shape, seed):
            """layers.Conv2D's glorot uniform over [height, width, in, out]: fan_in = height width in, fan_out = height
            width out"""
            field = shape[0] * shape[1]
            lim = float(np.sqrt(6.0 / (field * shape[2] + field * shape[3])))
            return get_initializer("uniform", lim, seed=seed)(shape)

        values = [embed([self.users_num, d]), embed([self.items_num, d]), embed([self.items_num, 2 * d]),
                  np.zeros(self.items_num, np.float32), conv([L, 1, 1, nv], 2018), np.zeros(nv, np.float32)]
        for i in range(1, L + 1):                                       # creation order of Caser.py:70-95
            values += [conv([i, d, 1, nh], 2018 + 10 * i), np.zeros(nh, np.float32)]
        values += [dense([nv * d + nh * L, d]), np.zeros(d, np.float32)]
        self.engine = CaserEngine(dict(zip(table_names(L), values)), self.lr, self.l2_reg, self.batch_size, self.seq_T,
                                  self.neg_samples, nv, nh, self.dropout)
        counts = np.zeros(self.users_num, np.int64)
        for u, items in self.user_pos_train.items():
            counts[u] = len(items)
        seq_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        flat = [i for u in range(self.users_num) for i in self.user_pos_train.get(u, ())]
        self.engine.set_sequences(seq_ptr, np.asarray(flat, np.int32))

    def train_model(self):
        import torch
        engine = self.engine
        self.logger.info(self.evaluator.metrics_info())
        self.logger.info(DEVIATIONS)
        users_list, item_seq_list, item_pos_list = self._generate_sequences()
        for epoch in range(self.epochs):
            users, seq, pos, neg, rows = epoch_feeds(users_list, item_seq_list, item_pos_list, self.user_pos_train,
                                                     self.items_num, self.neg_samples, self.batch_size)
            losses = torch.zeros((max(len(users), 1), 2), device=engine.item_embeddings.device)
            engine.run_schedule(users, seq, pos, neg, losses, rows)
            result = self.evaluate_model()
            self.logger.info("epoch %d:\t%s" % (epoch, result))

    def _generate_sequences(self):
        users_list, item_seq_list, item_pos_list, self.user_test_seq = generate_sequences(
            self.user_pos_train, self.items_num, self.seq_L, self.seq_T)
        return users_list, item_seq_list, item_pos_list

    def _sample_negative(self, users_list):
        return sample_negative(users_list, self.user_pos_train, self.items_num, self.neg_samples)

    def evaluate_model(self):
        return self.evaluator.evaluate(self)

    def predict(self, users, items=None):
        """Full mode: the [B, num_items] score rows as a device tensor (the evaluator's score-matrix path reads it in
        place).  Candidate mode: a list of per-user numpy arrays, the candidates' entries of those rows."""
        ratings = self.engine.score(np.asarray(list(users), dtype=np.int32))
        if items is None:
            return ratings
        host = ratings.cpu().numpy()
        return [host[k, np.asarray(its, dtype=np.int64)] for k, its in enumerate(items)]
