"""GRU4RecPlus on the HIP engine.

Reference: Balázs Hidasi and Alexandros Karatzoglou, "Recurrent Neural Networks with Top-k Gains for Session-based
Recommendations." in CIKM 2018.
Plugin-compatible with model/sequential_recommender/GRU4RecPlus.py: same constructor, config keys
(conf/GRU4RecPlus.properties: lr, reg, bpr_reg, layers, batch_size, loss, hidden_act, final_act, n_sample, sample_alpha,
epochs), the same ValueError texts for an unknown hidden_act / final_act / loss, log lines and `predict` contract.  The
per-step `sess.run([update_opt, final_state])` is neurec_amd/gru4recplus.py (csrc/gru4recplus.hip).  The
session-parallel bookkeeping of an epoch is GRU4Rec's `session_parallel_schedule`; the data, the initial values, the
evaluation and predict() are the GRU4Rec plugin's (the two reference classes compute them alike).

The sampler stays on the host and follows the reference's numpy stream exactly: `pop_cumsum` is built with the
reference's own expressions (GRU4RecPlus.py:59-62); per epoch the permutation is drawn first, then ONE
`np.random.rand(S * n_sample)` reshaped [S, n_sample] — the same stream as the reference's S successive
`np.random.rand(n_sample)` calls — and `np.searchsorted` (GRU4RecPlus.py:153-155).  The epoch's Y [S, B + n_sample] is
uploaded with the schedule, in chunks of steps when it is larger than Y_UPLOAD_BYTES.

Kept, as the class has it: `pop` comes from `np.unique` over the train events, so a sampled value is a RANK in the
sorted list of the items that occur in training, and the reference feeds that rank as an item id.  When every item
occurs in training the two coincide; when not, the ranks are fed as ids here too, so that the reference's traces are
reproducible.  The evaluation runs before every epoch's log line; no loss is logged.

Deviations, on purpose — GRU4Rec's three and one more:
  * a user without train items scores final_act(b), the zero state's row;
  * batch_size larger than the number of users with a train item is refused by name;
  * a multi-rank run is refused by name;
  * batch_size + n_sample < 2 is refused by name (the reference's softmax over no negative divides 0 by 0).
"""
import numpy as np

from ...util.tool import get_initializer
from .._common import require_single_gpu
from ..AbstractRecommender import SeqAbstractRecommender
from .GRU4Rec import DEVIATIONS, GRU4Rec, session_parallel_schedule

RANKS_AS_IDS = "negatives are sampled as ranks among the items that occur in training and fed as item ids, as the " \
               "reference does (%d of %d items occur)"
Y_UPLOAD_BYTES = 64 << 20           # an epoch's Y above this many bytes is uploaded and run in chunks of steps


def popularity_cumsum(data_items, sample_alpha):
    """GRU4RecPlus.py:59-62, the reference's own expressions"""
    _, pop = np.unique(data_items, return_counts=True)
    pop = np.power(pop, sample_alpha)
    pop_cumsum = np.cumsum(pop)
    return pop_cumsum / pop_cumsum[-1]


def epoch_feeds(offset_idx, data_items, pop_cumsum, batch_size, n_sample):
    """The feeds of one epoch from numpy's global stream, in the reference's order (GRU4RecPlus.py:165, 179): the
    permutation, then the negatives of all S steps in one draw.  Returns (X [S, B], Y [S, B + n_sample], reset [S, B])."""
    user_idx = np.random.permutation(len(offset_idx) - 1)
    X, Y, reset = session_parallel_schedule(offset_idx, user_idx, batch_size, data_items)
    if n_sample:
        S = len(X)
        neg = np.searchsorted(pop_cumsum, np.random.rand(S * n_sample).reshape(S, n_sample))
        Y = np.hstack([Y, neg.astype(np.int32)])
    return X, Y, reset


class GRU4RecPlus(GRU4Rec):
    def __init__(self, sess, dataset, conf):
        SeqAbstractRecommender.__init__(self, dataset, conf)
        self.train_matrix = dataset.train_matrix
        self.dataset = dataset
        self.users_num, self.items_num = self.train_matrix.shape
        self.lr = conf["lr"]
        self.reg = conf["reg"]
        self.layers = list(conf["layers"])
        self.batch_size = conf["batch_size"]
        self.n_sample = conf["n_sample"]
        self.sample_alpha = conf["sample_alpha"]
        self.epochs = conf["epochs"]
        self.bpr_reg = conf["bpr_reg"]
        self.hidden_act, self.final_act, self.loss = conf["hidden_act"], conf["final_act"], conf["loss"]
        if self.hidden_act not in ("relu", "tanh"):
            raise ValueError("There is not hidden_act named '%s'." % self.hidden_act)      # GRU4RecPlus.py:37
        if self.final_act not in ("relu", "linear", "leaky_relu"):
            raise ValueError("There is not final_act named '%s'." % self.final_act)        # GRU4RecPlus.py:47
        if self.loss not in ("bpr_max", "top1_max"):
            raise ValueError("There is not loss named '%s'." % self.loss)                  # GRU4RecPlus.py:54
        self.data_uit, self.offset_idx = self._init_data()
        self.pop_cumsum = popularity_cumsum(self.data_uit[:, 1], self.sample_alpha)
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...gru4recplus import GRU4RecPlusEngine
        require_single_gpu("GRU4RecPlus")
        n_present = len(self.offset_idx) - 1
        if self.batch_size > n_present:
            raise ValueError("GRU4RecPlus: batch_size=%d is larger than the %d users with a train item: the "
                             "session-parallel loop needs one session per slot" % (self.batch_size, n_present))
        if self.batch_size + self.n_sample < 2:
            raise ValueError("GRU4RecPlus: batch_size + n_sample = %d: a row needs at least one negative (the "
                             "reference divides 0 by 0)" % (self.batch_size + self.n_sample))
        embed = get_initializer("tnormal", 0.01, seed=2017)          # creation order of GRU4RecPlus.py:84-89
        kernel = get_initializer("xavier_uniform", 0.01, seed=2018)
        E_in = embed([self.items_num, self.layers[0]])
        Q = embed([self.items_num, self.layers[-1]])
        b = np.zeros(self.items_num, np.float32)
        cells, n_in = [], self.layers[0]
        for n in self.layers:
            cells.append((kernel([n_in + n, 2 * n]), np.ones(2 * n, np.float32), kernel([n_in + n, n]),
                          np.zeros(n, np.float32)))
            n_in = n
        self.engine = GRU4RecPlusEngine(E_in, Q, b, cells, self.lr, self.reg, self.batch_size, loss=self.loss,
                                        hidden_act=self.hidden_act, final_act=self.final_act, bpr_reg=self.bpr_reg,
                                        n_sample=self.n_sample)
        counts = np.bincount(self.data_uit[:, 0], minlength=self.users_num)
        seq_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.engine.set_sequences(seq_ptr, self.data_uit[:, 1])

    # ---------- training process -------
    def train_model(self):
        import torch
        engine = self.engine
        self.logger.info(self.evaluator.metrics_info())
        self.logger.info(DEVIATIONS)
        self.logger.info(RANKS_AS_IDS % (len(self.pop_cumsum), self.items_num))
        data_items = self.data_uit[:, 1]
        per_step = 4 * (self.batch_size + self.n_sample)
        chunk = max(1, Y_UPLOAD_BYTES // per_step)
        for epoch in range(self.epochs):
            X, Y, reset = epoch_feeds(self.offset_idx, data_items, self.pop_cumsum, self.batch_size, self.n_sample)
            losses = torch.zeros((max(len(X), 1), 2), device=engine.E_in.device)
            engine.reset_states()
            for s0 in range(0, len(X), chunk):
                s1 = s0 + chunk
                engine.run_schedule(X[s0:s1], Y[s0:s1], reset[s0:s1], losses[s0:s1])
            result = self.evaluate_model()
            self.logger.info("epoch %d:\t%s" % (epoch, result))
