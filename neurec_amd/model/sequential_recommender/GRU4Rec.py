"""GRU4Rec on the HIP engine.

Reference: Balázs Hidasi et al., "Session-based Recommendations with Recurrent Neural Networks." in ICLR 2016.
Plugin-compatible with model/sequential_recommender/GRU4Rec.py: same constructor, config keys
(conf/GRU4Rec.properties: lr, reg, layers, batch_size, loss, hidden_act, final_act, epochs), the same ValueError texts
for an unknown hidden_act / final_act / loss, log lines and `predict` contract.  The per-step
`sess.run([update_opt, final_state])` is neurec_amd/gru4rec.py (csrc/gru4rec.hip); the recurrent states stay on the
device between steps, and the session-parallel bookkeeping of an epoch (GRU4Rec.py:134-174) is worked out on the host
up front by `session_parallel_schedule`, uploaded once and issued with no host round trip.

Initial values: E_in and Q truncated normal with sigma 0.01, b zeros, the cells' kernels Glorot uniform (TF's default
for get_variable), the gate biases ones, the candidate biases zeros.  TF's Philox stream cannot be reproduced: the draws
come from the project's `get_initializer` with seed 2017 (embeddings) and 2018 (kernels), numpy's stream.

Kept, as the class has them: the evaluation runs before every epoch's log line (there is no `verbose` key) from user
vectors that are the top layer's output after the user's whole train sequence; no loss is logged.

Deviations, on purpose:
  * a user without train items scores final_act(b) — the zero state's row (the reference mis-indexes offset_idx for
    such a user);
  * batch_size larger than the number of users with a train item is refused by name (the reference raises IndexError);
  * a multi-rank run is refused by name.
Candidate mode returns the candidates' entries of the full-mode rows.
"""
import numpy as np

from ...util.tool import get_initializer
from .._common import require_single_gpu
from ..AbstractRecommender import SeqAbstractRecommender

DEVIATIONS = "users without train items score final_act(b), the zero state's row (the reference mis-indexes " \
             "offset_idx for such a user)"


def session_parallel_schedule(offset_idx, user_idx, batch_size, data_items=None):
    """The feeds of one epoch of the session-parallel loop (GRU4Rec.py:141-174) without running a step.

    offset_idx [n + 1]: where each user's events begin in the (user, time)-sorted event list; user_idx: the epoch's
    permutation of the n users.  Returns (X [S, B], Y [S, B], reset [S, B] uint8): step s feeds the events at positions
    X[s] and asks for those at Y[s] = X[s] + 1 (with `data_items` given, the items at those positions instead), and
    reset[s] marks the slots whose state is zeroed after step s — every slot whose session ran out, refilled or not.
    A round whose shortest session has one event left runs no step and only refills; when the next user would pass the
    end of the permutation the epoch ends at once, sessions in flight abandoned."""
    offset_idx = np.asarray(offset_idx, dtype=np.int64)
    user_idx = np.asarray(user_idx, dtype=np.int64)
    n_users, B = len(offset_idx) - 1, int(batch_size)
    if B < 1:
        raise ValueError("GRU4Rec: batch_size must be at least 1")
    if B > n_users:
        raise ValueError("GRU4Rec: batch_size=%d is larger than the %d users with a train item: the session-parallel "
                         "loop needs one session per slot" % (B, n_users))
    pos = offset_idx[user_idx[:B]].copy()
    end = offset_idx[user_idx[:B] + 1].copy()
    taken = B                                             # users handed to a slot so far
    X, reset = [], []
    while True:
        steps = int((end - pos).min()) - 1
        for i in range(steps):
            X.append(pos + i)
            reset.append(np.zeros(B, np.uint8))
        pos += max(steps, 0)
        out = np.flatnonzero(end - pos <= 1)
        room = n_users - taken
        for slot in out[:room]:
            u = user_idx[taken]
            pos[slot], end[slot] = offset_idx[u], offset_idx[u + 1]
            taken += 1
        if len(out) and reset:
            reset[-1][out] = 1
        if len(out) > room:
            break
    S = len(X)
    X = np.stack(X).astype(np.int64) if S else np.zeros((0, B), np.int64)
    reset = np.stack(reset) if S else np.zeros((0, B), np.uint8)
    Y = X + 1
    if data_items is not None:
        items = np.asarray(data_items)
        X, Y = items[X], items[Y]
    return X.astype(np.int32), Y.astype(np.int32), reset


class GRU4Rec(SeqAbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(GRU4Rec, self).__init__(dataset, conf)
        self.train_matrix = dataset.train_matrix
        self.dataset = dataset
        self.users_num, self.items_num = self.train_matrix.shape
        self.lr = conf["lr"]
        self.reg = conf["reg"]
        self.layers = list(conf["layers"])
        self.batch_size = conf["batch_size"]
        self.epochs = conf["epochs"]
        self.hidden_act, self.final_act, self.loss = conf["hidden_act"], conf["final_act"], conf["loss"]
        if self.hidden_act not in ("relu", "tanh"):
            raise ValueError("There is not hidden_act named '%s'." % self.hidden_act)      # GRU4Rec.py:34
        if self.final_act not in ("relu", "linear", "leaky_relu"):
            raise ValueError("There is not final_act named '%s'." % self.final_act)        # GRU4Rec.py:44
        if self.loss not in ("bpr", "top1"):
            raise ValueError("There is not loss named '%s'." % self.loss)                  # GRU4Rec.py:51
        self.data_uit, self.offset_idx = self._init_data()
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def _init_data(self):
        """(user, item, time) rows sorted by (user, time) — stably, from the time matrix's DOK order, which decides
        between equal timestamps — as int32, and the offset of every user PRESENT in the data (GRU4Rec.py:62-72)"""
        dok = self.dataset.time_matrix.todok()
        n = len(dok)
        coords = np.fromiter((c for rc in dok.keys() for c in rc), dtype=np.int64, count=2 * n).reshape(n, 2)
        times = np.fromiter(dok.values(), dtype=np.float64, count=n)
        order = np.lexsort((times, coords[:, 0]))                  # stable: ties keep the DOK order
        data_uit = np.empty((n, 3), dtype=np.int32)
        data_uit[:, 0], data_uit[:, 1] = coords[order, 0], coords[order, 1]
        data_uit[:, 2] = times[order].astype(np.int32)
        _, first = np.unique(data_uit[:, 0], return_index=True)
        offset_idx = np.append(first, n).astype(np.int32)
        return data_uit, offset_idx

    def build_graph(self):
        from ...gru4rec import GRU4RecEngine
        require_single_gpu("GRU4Rec")
        n_present = len(self.offset_idx) - 1
        if self.batch_size > n_present:
            raise ValueError("GRU4Rec: batch_size=%d is larger than the %d users with a train item: the "
                             "session-parallel loop needs one session per slot" % (self.batch_size, n_present))
        embed = get_initializer("tnormal", 0.01, seed=2017)          # creation order of GRU4Rec.py:80-85
        kernel = get_initializer("xavier_uniform", 0.01, seed=2018)
        E_in = embed([self.items_num, self.layers[0]])
        Q = embed([self.items_num, self.layers[-1]])
        b = np.zeros(self.items_num, np.float32)
        cells, n_in = [], self.layers[0]
        for n in self.layers:
            cells.append((kernel([n_in + n, 2 * n]), np.ones(2 * n, np.float32), kernel([n_in + n, n]),
                          np.zeros(n, np.float32)))
            n_in = n
        self.engine = GRU4RecEngine(E_in, Q, b, cells, self.lr, self.reg, self.batch_size, loss=self.loss,
                                    hidden_act=self.hidden_act, final_act=self.final_act)
        counts = np.bincount(self.data_uit[:, 0], minlength=self.users_num)
        seq_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.engine.set_sequences(seq_ptr, self.data_uit[:, 1])

    # ---------- training process -------
    def train_model(self):
        import torch
        engine = self.engine
        self.logger.info(self.evaluator.metrics_info())
        self.logger.info(DEVIATIONS)
        data_items = self.data_uit[:, 1]
        for epoch in range(self.epochs):
            user_idx = np.random.permutation(len(self.offset_idx) - 1)      # GRU4Rec.py:142: the global stream
            X, Y, reset = session_parallel_schedule(self.offset_idx, user_idx, self.batch_size, data_items)
            losses = torch.zeros((max(len(X), 1), 2), device=engine.E_in.device)
            engine.reset_states()
            engine.run_schedule(X, Y, reset, losses)
            result = self.evaluate_model()
            self.logger.info("epoch %d:\t%s" % (epoch, result))

    def evaluate_model(self):
        self.engine.user_states()             # every user's sequence from a zero state, once per evaluation
        return self.evaluator.evaluate(self)

    def get_eval_factors(self):
        """Device tables for the evaluator's on-GPU factor path, final_act linear: [H | 1] against [Q | b]; None for
        relu / leaky_relu, which are scored through predict()."""
        return self.engine.eval_factors()

    def predict(self, users, items=None):
        """Full mode: the [B, num_items] score rows as a device tensor (the evaluator's score-matrix path reads it in
        place).  Candidate mode: a list of per-user numpy arrays, the candidates' entries of those rows."""
        ratings = self.engine.score(np.asarray(list(users), dtype=np.int32))
        if items is None:
            return ratings
        host = ratings.cpu().numpy()
        return [host[k, np.asarray(its, dtype=np.int64)] for k, its in enumerate(items)]
