"""IRGAN on the HIP engine.

Reference: Jun Wang et al., "IRGAN: A Minimax Game for Unifying Generative and Discriminative Information Retrieval
Models." SIGIR 2017.
Plugin-compatible with model/general_recommender/IRGAN.py: same constructor, config keys (conf/IRGAN.properties:
factors_num, lr, g_reg, d_reg, epochs, g_epoch, d_epoch, batch_size, d_tau, topk, pretrain_file), schedule (`epochs`
times: d_epoch D passes, each with new data and a reshuffled DataIterator of batch_size that keeps the last short batch,
then g_epoch G passes, each followed by `evaluate()` logged as "%s") and `evaluate()` / `predict(users, items)`.  The data
of a D pass, the D steps, the G user steps and the scorer are neurec_amd/irgan.py (csrc/irgan.hip).

As the reference:
  * the train users are the rows for which `any(row.indices)` is true (IRGAN.py:142-147): a user without a train item is
    left out of both passes, and so is a user whose only train item is item 0, because any([0]) is false;
  * D's `pre_loss` is a vector, the per-example cross entropy plus the SCALAR regulariser, and `minimize` differentiates
    its sum: the regulariser counts B times, B the actual size of the batch (the short last batch uses its own);
  * the positives are not excluded from D's negatives: a draw from the generator may be a train item of the user;
  * the generator's sampling mixture is 0.8 p + 0.2 / deg on the positives, the 0.2 hard-coded (IRGAN.py:215), and
    there is no temperature in the G step; rewards are 2 (sigmoid - 1/2) p / pn, held constant in the gradient;
  * G's regulariser takes the user row once and every SAMPLED item row once per draw; the update of Q_g and b_g is dense,
    so the users of a G pass are strictly in sequence, in ascending id.

Deviations, on purpose:
  * the draws come from the device's counter-based generator, not from numpy's stream: a draw is a pure function of
    (seed, pass counter, phase, user, draw index), drawn from integer weights floor(exp((z - max z) / tau) 2^31);
  * the maximum logit is always subtracted, where the reference's unshifted `np.exp` overflows above 88;
  * an item whose probability is below 2^-31 of the largest has weight zero and is never drawn;
  * the initial values of D (and of G without a pretrain file) come from a numpy generator with a fixed seed:
    uniform(-0.05, 0.05) tables, zero biases, as GEN / DIS draw them with `param=None`;
  * a `pretrain_file` that exists is unpickled as the reference does, with encoding="latin", and its shapes are checked;
    one that is absent makes G start as `GEN` itself does with `param=None`, with one log line saying so, where the
    reference raises;
  * the train matrix is `dataset.train_matrix` (IRGAN.py:128 reads `trainMatrix`, a name the dataset no longer has);
  * limits: factors_num 1 to 128, batch_size 1 to 1,024, d_tau above 0, regularisers 0 or more, lr above 0; anything
    else is refused with the key and the range; multi-rank runs are refused;
  * predict() in full mode returns the [B, num_items] device tensor, in candidate mode per-user numpy arrays.
"""
import os
import pickle

import numpy as np

from ...util import DataIterator
from .._common import require_single_gpu
from ..AbstractRecommender import AbstractRecommender

INIT_DELTA = 0.05


def initial_tables(num_users, num_items, d, pretrain=None, seed=2017):
    """{g_P, g_Q, g_b, d_P, d_Q, d_b}: G from `pretrain` ([P, Q, b]) or as GEN draws it with param=None, D as DIS does"""
    rs = np.random.RandomState(seed)
    draw = lambda n: rs.uniform(-INIT_DELTA, INIT_DELTA, (n, d)).astype(np.float32)     # noqa: E731
    out = {"d_P": draw(num_users), "d_Q": draw(num_items), "d_b": np.zeros(num_items, np.float32)}
    if pretrain is None:
        out.update({"g_P": draw(num_users), "g_Q": draw(num_items), "g_b": np.zeros(num_items, np.float32)})
    else:
        if len(pretrain) != 3:
            raise ValueError("IRGAN: pretrain_file must hold [P, Q, b], got %d entries" % len(pretrain))
        P, Q, b = (np.asarray(x, dtype=np.float32) for x in pretrain)
        if P.shape != (num_users, d) or Q.shape != (num_items, d) or b.shape != (num_items,):
            raise ValueError("IRGAN: pretrain_file holds P %s, Q %s, b %s; [%d, %d], [%d, %d], [%d] expected" % (
                list(P.shape), list(Q.shape), list(b.shape), num_users, d, num_items, d, num_items))
        out.update({"g_P": P, "g_Q": Q, "g_b": b})
    return {k: out[k] for k in ("g_P", "g_Q", "g_b", "d_P", "d_Q", "d_b")}


class IRGAN(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(IRGAN, self).__init__(dataset, conf)
        self.train_matrix = dataset.train_matrix.tocsr()
        self.num_users, self.num_items = self.train_matrix.shape
        self.factors_num = conf["factors_num"]
        self.lr = conf["lr"]
        self.g_reg = conf["g_reg"]
        self.d_reg = conf["d_reg"]
        self.epochs = conf["epochs"]
        self.g_epoch = conf["g_epoch"]
        self.d_epoch = conf["d_epoch"]
        self.batch_size = conf["batch_size"]
        self.d_tau = conf["d_tau"]
        self.topK = conf["topk"]
        self.pretrain_file = conf["pretrain_file"]
        self.dataset = dataset
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def load_pretrain(self):
        """[P, Q, b] of the pretrain file, or None (with one log line) when there is no such file"""
        path = self.pretrain_file
        if not (isinstance(path, str) and os.path.isfile(path)):
            self.logger.info("IRGAN: pretrain_file %r does not exist; the generator starts from uniform(-%g, %g)"
                             % (path, INIT_DELTA, INIT_DELTA))
            return None
        with open(path, "rb") as fin:
            return pickle.load(fin, encoding="latin")

    def build_graph(self):
        from ...irgan import IRGANEngine, check_config
        require_single_gpu("IRGAN")
        check_config(self.factors_num, self.batch_size, self.d_tau, self.g_reg, self.d_reg, self.lr)
        tables = initial_tables(self.num_users, self.num_items, int(self.factors_num), self.load_pretrain())
        self.engine = IRGANEngine(tables, self.train_matrix, self.lr, self.g_reg, self.d_reg, self.d_tau,
                                  self.batch_size, seed=2018)

    def train_model(self):
        for _ in range(self.epochs):
            for _ in range(self.d_epoch):
                self.training_discriminator()
            for _ in range(self.g_epoch):
                self.training_generator()
                self.logger.info("%s" % (self.evaluate()))

    def training_discriminator(self):
        engine = self.engine
        data_iter = DataIterator(np.arange(engine.d_pass_size()), batch_size=self.batch_size, shuffle=True,
                                 drop_last=False)
        batches = [np.asarray(idx, dtype=np.int32).reshape(-1) for idx in data_iter]
        engine.d_pass(np.concatenate(batches) if batches else np.zeros(0, np.int32))

    def training_generator(self):
        self.engine.g_pass()

    def evaluate(self):
        return self.evaluator.evaluate(self)

    def predict(self, users, items=None):
        """Full mode: the [B, num_items] score rows as a device tensor.  Candidate mode: a list of per-user numpy
        arrays."""
        users = np.asarray(list(users), dtype=np.int32)
        if items is None:
            return self.engine.score(users)
        sizes = [len(its) for its in items]
        flat = np.concatenate([np.asarray(its, dtype=np.int32).reshape(-1) for its in items]) if sizes \
            else np.zeros(0, np.int32)
        out = self.engine.forward(users, flat, sizes).cpu().numpy()
        return np.split(out, np.cumsum(sizes)[:-1]) if sizes else []
