"""SRGNN on the HIP engine.

Reference: Shu Wu, Yuyuan Tang, Yanqiao Zhu, Liang Wang, Xing Xie, and Tieniu Tan, "Session-Based Recommendation with
Graph Neural Networks." in AAAI 2019.
Plugin-compatible with model/sequential_recommender/SRGNN.py: same constructor, config keys (conf/SRGNN.properties: lr,
L2, hidden_size, step, batch_size, epochs, lr_dc, lr_dc_step, nonhybrid, max_seq_len), log lines and `predict` contract.
The per-step `sess.run(self.train_opt)` is neurec_amd/srgnn.py (csrc/srgnn.hip).

The samples are the reference's (SRGNN.py:33-38): per user and i in 1 .. len - 1 the session seqs[-i - max_seq_len:-i]
with target seqs[-i], kept here as the pair (user, end = len - i) over the sequences resident on the device.  The epoch
order follows the reference on numpy's global stream (SRGNN.py:144-174): the sample indices sorted by session length,
descending and stable, cut into chunks of 32 batch_size; one permutation of the chunks, then one permutation inside each
chunk as it is reached, batched with drop_last.  The learning rate is tf.train.exponential_decay's staircase in float32
over the global step.  The initial values come from `get_initializer` with fixed seeds in the creation order of the
variables: uniform(+-1 / sqrt(hidden_size)) — b_in and b_out too, nasr_b zeros — and for the GRUCell glorot-uniform
kernels, a gate bias of ones and a candidate bias of zeros.

Deviations, on purpose:
  * a user without train items scores a zero row (the reference raises KeyError);
  * a multi-rank run is refused by name.
"""
import numpy as np

from ...util.tool import csr_to_user_dict_bytime, get_initializer
from .._common import require_single_gpu
from ..AbstractRecommender import SeqAbstractRecommender

DEVIATIONS = "users without train items score a zero row (the reference raises KeyError)"


def train_samples(user_pos_train, max_seq_len):
    """SRGNN.py:33-38 as (users, ends, lengths): sample k is the session seqs[max(0, end - max_seq_len):end] of user
    users[k] with target seqs[end]"""
    users, ends, lengths = [], [], []
    for user, seqs in user_pos_train.items():
        n = len(seqs)
        for i in range(1, n):
            users.append(user)
            ends.append(n - i)
            lengths.append(len(seqs[-i - max_seq_len:-i]))
    return np.asarray(users, np.int32), np.asarray(ends, np.int32), np.asarray(lengths, np.int64)


def epoch_feeds(lengths, batch_size):
    """The sample indices of one epoch's batches [S, batch_size] in the reference's numpy stream order
    (SRGNN.py:145-147, 166-174)"""
    lengths = np.asarray(lengths)
    by_length = np.argsort(-lengths, kind="stable")                 # sorted(..., reverse=True) keeps ties in order
    size = 32 * batch_size
    chunks = [by_length[k:k + size] for k in range(0, len(by_length), size)]
    batches = []
    for c in np.random.permutation(len(chunks)):                    # DataIterator(index_chunks, shuffle=True)
        idx = chunks[c]
        order = np.random.permutation(len(idx))                     # DataIterator(indexes, shuffle=True, drop_last=True)
        for k in range(len(idx) // batch_size):
            batches.append(idx[order[k * batch_size:(k + 1) * batch_size]])
    return np.asarray(batches, np.int64).reshape(len(batches), batch_size)


def learning_rates(lr, lr_dc, lr_dc_step, n_samples, batch_size, first, n_steps):
    """tf.train.exponential_decay(lr, global_step, decay_steps = lr_dc_step n_samples / batch_size, lr_dc,
    staircase=True) for global_step first .. first + n_steps - 1: the divide, the floor and the power in float32"""
    decay_steps = np.float32(lr_dc_step * n_samples / batch_size)
    out = np.zeros(n_steps, np.float32)
    for k in range(n_steps):                  # scalar by scalar: numpy's array power may differ from powf by an ulp
        p = np.floor(np.float32(first + k) / decay_steps)
        out[k] = np.float32(lr) * np.power(np.float32(lr_dc), p, dtype=np.float32)
    return out


def initial_values(num_items, hidden_size):
    """{name: float32 array} in creation order"""
    from ...srgnn import TABLES, shapes
    d = hidden_size
    stdv = 1.0 / np.sqrt(d)
    out = {}
    for k, name in enumerate(TABLES):
        shape = shapes(num_items, d)[name]
        if name == "nasr_b" or name == "candidate_bias":
            out[name] = np.zeros(shape, np.float32)
        elif name == "gates_bias":
            out[name] = np.ones(shape, np.float32)                  # GRUCell's bias_initializer default: ones
        elif name.endswith("_kernel"):
            out[name] = get_initializer("xavier_uniform", 0.01, seed=2017 + k)(shape)     # get_variable's default
        else:
            out[name] = get_initializer("uniform", stdv, seed=2017 + k)(shape)
    return out


class SRGNN(SeqAbstractRecommender):
    def __init__(self, sess, dataset, config):
        super(SRGNN, self).__init__(dataset, config)
        self.lr = config["lr"]
        self.L2 = config["L2"]
        self.hidden_size = config["hidden_size"]
        self.step = config["step"]
        self.batch_size = config["batch_size"]
        self.epochs = config["epochs"]
        self.lr_dc = config["lr_dc"]
        self.lr_dc_step = config["lr_dc_step"]
        self.nonhybrid = config["nonhybrid"]
        self.max_seq_len = config["max_seq_len"]
        self.num_users, self.num_item = dataset.train_matrix.shape
        self.user_pos_train = csr_to_user_dict_bytime(dataset.time_matrix, dataset.train_matrix)
        self.train_users, self.train_ends, self.train_lengths = train_samples(self.user_pos_train, self.max_seq_len)
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None
        self.global_step = 0

    def build_graph(self):
        from ...srgnn import SRGNNEngine
        require_single_gpu("SRGNN")
        self.engine = SRGNNEngine(initial_values(self.num_item, self.hidden_size), self.lr, self.L2, self.batch_size,
                                  self.max_seq_len, self.step, self.nonhybrid)
        counts = np.zeros(self.num_users, np.int64)
        for u, items in self.user_pos_train.items():
            counts[u] = len(items)
        seq_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        flat = [i for u in range(self.num_users) for i in self.user_pos_train.get(u, ())]
        self.engine.set_sequences(seq_ptr, np.asarray(flat, np.int32))

    def train_model(self):
        import torch
        engine = self.engine
        self.logger.info(self.evaluator.metrics_info())
        self.logger.info(DEVIATIONS)
        for epoch in range(self.epochs):
            batches = epoch_feeds(self.train_lengths, self.batch_size)
            S = len(batches)
            lrs = learning_rates(self.lr, self.lr_dc, self.lr_dc_step, len(self.train_users), self.batch_size,
                                 self.global_step, S)
            losses = torch.zeros((max(S, 1), 2), device=engine.T["embedding"].device)
            if S:
                engine.run_schedule(self.train_users[batches], self.train_ends[batches], losses, lrs)
            self.global_step += S
            self.logger.info("epoch %d:\t%s" % (epoch, self.evaluate_model()))

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
