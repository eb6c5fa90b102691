"""CDAE on the HIP engine.

Reference: Yao Wu et al., "Collaborative Denoising Auto-Encoders for Top-N Recommender Systems." in WSDM 2016.
Plugin-compatible with model/general_recommender/CDAE.py: same constructor, config keys (conf/CDAE.properties: lr, reg,
hidden_dim, dropout, num_neg, epochs, batch_size, hidden_act, loss_func), log lines (`metrics_info()` once, then
`epoch %d:\\t%s` after every epoch, counting from 0) and `predict` contract.  The per-user batch loops and the
`sess.run(self.train_opt)` of every step are neurec_amd/cdae.py (csrc/cdae.hip).

As the reference:
  * the negatives of a user are written into the INPUT row as well (CDAE.py:118): the encoder pools the positives and
    the negatives, all with value 1, and the corruption drops among both;
  * predict() corrupts too: the keep probability is the config value, not the fed placeholder (CDAE.py:63), so
    evaluation sees train rows with `dropout` of their entries dropped and the rest scaled by 1 / (1 - dropout);
    `CDAEEngine.score(users, keep_prob=1.0)` gives the uncorrupted scores;
  * the regulariser takes every item row of a batch ONCE (`tf.unique(items_ph)`, CDAE.py:83), however many users hold
    the item and whether as a positive or a negative; the user rows per occurrence; all of `en_offset`;
  * the optimiser is Adam whatever else is configured; the users with a train item are shuffled once per epoch on
    numpy's global stream and the last short batch is kept.

Deviations, on purpose:
  * the draws and the corruption masks come from the device's counter-based generators, not from glibc rand() and
    TensorFlow's stream; a draw is keyed by (step seed, user, draw index);
  * the initial values come from numpy generators with fixed seeds (truncated normal 0.01 in the creation order of the
    variables; `en_offset` and `item_bias` zero);
  * multi-rank runs are refused; `num_neg < 1` and `hidden_dim` outside 1..128 are refused with a reason;
  * predict() in full mode returns the [B, num_items] device tensor, in candidate mode per-user numpy arrays.
"""
import numpy as np

from ...util import DataIterator
from ...util.tool import get_initializer
from .._common import require_single_gpu
from ..AbstractRecommender import AbstractRecommender


def initial_variables(num_users, num_items, hidden_dim):
    """{name: array} in the reference's creation order (CDAE.py:54-60)"""
    init = get_initializer("tnormal", 0.01, seed=2017)
    return {"user_embeddings": init([num_users, hidden_dim]), "en_embeddings": init([num_items, hidden_dim]),
            "en_offset": np.zeros(hidden_dim, np.float32), "de_embeddings": init([num_items, hidden_dim]),
            "de_bias": np.zeros(num_items, np.float32)}


class CDAE(AbstractRecommender):
    def __init__(self, sess, dataset, config):
        super(CDAE, self).__init__(dataset, config)
        from ...cdae import ACTS
        self.emb_size = config["hidden_dim"]
        self.lr = config["lr"]
        self.reg = config["reg"]
        self.dropout = config["dropout"]
        self.loss_func = config["loss_func"]
        self.num_neg = config["num_neg"]
        self.epochs = config["epochs"]
        self.batch_size = config["batch_size"]
        self.hidden_act = config["hidden_act"]
        self.dataset = dataset
        self.train_csr_mat = dataset.train_matrix.tocsr()
        self.num_users, self.num_items = dataset.num_users, dataset.num_items
        if self.hidden_act not in ACTS:                          # CDAE.py:36-41 raises in the constructor
            raise ValueError(f"hidden activate function {self.hidden_act} is invalid.")
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...cdae import CDAEEngine, check_config
        require_single_gpu("CDAE")
        check_config(self.hidden_act, self.loss_func, self.num_neg, self.emb_size)
        self.engine = CDAEEngine(initial_variables(self.num_users, self.num_items, int(self.emb_size)),
                                 self.train_csr_mat, self.lr, self.reg, self.dropout, self.num_neg, self.batch_size,
                                 hidden_act=self.hidden_act, loss_func=self.loss_func, seed=2018)

    def train_model(self):
        import torch
        engine = self.engine
        counts = np.diff(self.train_csr_mat.indptr)
        train_users = [user for user in range(self.num_users) if counts[user]]
        user_iter = DataIterator(train_users, batch_size=self.batch_size, shuffle=True, drop_last=False)
        self.logger.info(self.evaluator.metrics_info())
        self.losses = losses = torch.zeros((max(len(user_iter), 1), 2), device=engine.T["en_offset"].device)
        for epoch in range(self.epochs):
            for n, bat_users in enumerate(user_iter):
                engine.step(np.asarray(bat_users, dtype=np.int32), losses[n])
            result = self.evaluate_model()
            self.logger.info("epoch %d:\t%s" % (epoch, result))

    def evaluate_model(self):
        return self.evaluator.evaluate(self)

    def predict(self, users, items=None):
        """Full mode: the [B, num_items] score rows as a device tensor (the evaluator's score-matrix path reads it in
        place).  Candidate mode: a list of per-user numpy arrays.  Both from train rows corrupted at the config's
        dropout, as the reference's graph has it."""
        users = np.asarray(list(users), dtype=np.int32)
        if items is None:
            return self.engine.score(users)
        sizes = [len(its) for its in items]
        flat = np.concatenate([np.asarray(its, dtype=np.int32).reshape(-1) for its in items]) if sizes \
            else np.zeros(0, np.int32)
        out = self.engine.forward(users, flat, sizes).cpu().numpy()
        return np.split(out, np.cumsum(sizes)[:-1]) if sizes else []
