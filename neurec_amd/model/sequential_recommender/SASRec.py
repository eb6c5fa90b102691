"""SASRec on the HIP engine.

Reference: Wang-Cheng Kang and Julian McAuley, "Self-Attentive Sequential Recommendation." in ICDM 2018.
Plugin-compatible with model/sequential_recommender/SASRec.py: same constructor, config keys (conf/SASRec.properties:
lr, l2_emb, hidden_units, dropout_rate, max_len, num_blocks, num_heads, batch_size, epochs), log lines and `predict`
contract.  The per-step `sess.run(self.train_opt)` is neurec_amd/sasrec.py (csrc/sasrec.hip).

The feeds follow the reference's order on numpy's global stream (SASRec.py:393-395): `get_train_data` first — users in
chunks of 1024, seq = items[:-1], pos = items[1:], the negatives from `batch_randint_choice(I, lens, replace=True,
exclusion=all train items)`, all three `pad_sequences(value=I, max_len=L, padding='pre', truncating='pre')` — then
`DataIterator(shuffle=True)`'s permutation.  The initial values come from `get_initializer` with fixed seeds in the
creation order of the variables; the dropout masks from the engine's counter-based device generator.

Deviations, on purpose:
  * a multi-rank run is refused by name;
  * hidden_units % num_heads != 0 is a ValueError (TF's split raises there);
  * a batch with sum(is_target) == 0 makes the reference divide 0 by 0 and poison every variable: here that step is
    skipped and counted;
  * the reference's sampler raises for a user with one train item (a request of size 0) and returns a bare int for a
    user with two, which pad_sequences cannot take: here the first is an all-padded row and the second a one-item list;
  * a user without train items scores the all-padded row, final-ln beta . table^T (the reference raises KeyError).
"""
import numpy as np

from ...util import DataIterator, batch_randint_choice, pad_sequences
from ...util.tool import csr_to_user_dict_bytime, get_initializer
from .._common import require_single_gpu
from ..AbstractRecommender import SeqAbstractRecommender

DEVIATIONS = "steps whose batch has no target are skipped and counted (the reference divides 0 by 0); users with one " \
             "or two train items are padded rows (the reference's sampler stops on them); users without train items " \
             "score the all-padded row"


def get_train_data(user_pos_train, items_num, max_len, sampler=batch_randint_choice):
    """SASRec.get_train_data (SASRec.py:407-425) as arrays [n_users_present, max_len]"""
    seq_list, pos_list, neg_list = [], [], []
    for bat_users in DataIterator(list(user_pos_train.keys()), batch_size=1024, shuffle=False):
        bat_seq = [user_pos_train[u][:-1] for u in bat_users]
        bat_pos = [user_pos_train[u][1:] for u in bat_users]
        sizes = [len(p) for p in bat_pos]
        exclusion = [user_pos_train[u] for u in bat_users]
        ask = [k for k, n in enumerate(sizes) if n > 0]                 # the reference's sampler raises on size 0
        drawn = sampler(items_num, [sizes[k] for k in ask], replace=True, exclusion=[exclusion[k] for k in ask]) \
            if ask else []
        bat_neg = [[] for _ in sizes]
        for k, got in zip(ask, drawn):
            bat_neg[k] = list(got) if isinstance(got, (list, tuple, np.ndarray)) else [got]   # ... and unwraps size 1
        for out, rows in ((seq_list, bat_seq), (pos_list, bat_pos), (neg_list, bat_neg)):
            out.extend(pad_sequences(rows, value=items_num, max_len=max_len, padding="pre", truncating="pre"))
    shape = (len(seq_list), max_len)
    return tuple(np.asarray(a, np.int32).reshape(shape) for a in (seq_list, pos_list, neg_list))


def epoch_feeds(user_pos_train, items_num, max_len, batch_size, sampler=batch_randint_choice):
    """The feeds of one epoch in the reference's numpy stream order: get_train_data first, then the shuffle.  Returns
    (seq, pos, neg) int32 [S, batch_size, max_len] — the last batch filled up with all-padded rows, which are no work
    and no target — and rows [S], the true size of each batch."""
    seq, pos, neg = get_train_data(user_pos_train, items_num, max_len, sampler)
    n = len(seq)
    order = np.random.permutation(n) if n else np.zeros(0, np.int64)    # DataIterator(shuffle=True)
    S = (n + batch_size - 1) // batch_size
    out = [np.full((S, batch_size, max_len), items_num, np.int32) for _ in range(3)]
    rows = np.zeros(S, np.int32)
    for s in range(S):
        idx = order[s * batch_size:(s + 1) * batch_size]
        rows[s] = len(idx)
        for o, a in zip(out, (seq, pos, neg)):
            o[s, :len(idx)] = a[idx]
    return out[0], out[1], out[2], rows


class SASRec(SeqAbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(SASRec, self).__init__(dataset, conf)
        train_matrix, time_matrix = dataset.train_matrix, dataset.time_matrix
        self.dataset = dataset
        self.users_num, self.items_num = train_matrix.shape
        self.lr = conf["lr"]
        self.l2_emb = conf["l2_emb"]
        self.hidden_units = conf["hidden_units"]
        self.batch_size = conf["batch_size"]
        self.epochs = conf["epochs"]
        self.dropout_rate = conf["dropout_rate"]
        self.max_len = conf["max_len"]
        self.num_blocks = conf["num_blocks"]
        self.num_heads = conf["num_heads"]
        if self.hidden_units % self.num_heads:
            raise ValueError("SASRec: num_heads=%d does not divide hidden_units=%d" % (self.num_heads, self.hidden_units))
        self.user_pos_train = csr_to_user_dict_bytime(time_matrix, train_matrix)
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...sasrec import SASRecEngine
        require_single_gpu("SASRec")
        d, L = self.hidden_units, self.max_len
        embed = get_initializer("xavier_uniform", 0.01, seed=2017)      # get_variable's default: glorot uniform
        kernel = get_initializer("xavier_uniform", 0.01, seed=2018)     # layers.dense / conv1d: glorot uniform
        zeros, ones = (lambda: np.zeros(d, np.float32)), (lambda: np.ones(d, np.float32))
        item_emb, pos_emb = embed([self.items_num, d]), embed([L, d])   # creation order of SASRec.py:299-356
        blocks = []
        for _ in range(self.num_blocks):
            blocks.append([zeros(), ones(), kernel([d, d]), zeros(), kernel([d, d]), zeros(), kernel([d, d]), zeros(),
                           zeros(), ones(), kernel([d, d]), zeros(), kernel([d, d]), zeros()])
        self.engine = SASRecEngine(item_emb, pos_emb, blocks, (zeros(), ones()), self.lr, self.l2_emb, self.batch_size,
                                   self.num_heads, self.dropout_rate)
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
        for epoch in range(self.epochs):
            seq, pos, neg, _ = epoch_feeds(self.user_pos_train, self.items_num, self.max_len, self.batch_size)
            losses = torch.zeros((max(len(seq), 1), 2), device=engine.item_emb.device)
            engine.run_schedule(seq, pos, neg, losses)
            result = self.evaluate_model()
            self.logger.info("epoch %d:\t%s" % (epoch, result))
        if engine.skipped_steps:
            self.logger.info("%d steps without a target were skipped" % engine.skipped_steps)

    def get_train_data(self):
        return get_train_data(self.user_pos_train, self.items_num, self.max_len)

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
