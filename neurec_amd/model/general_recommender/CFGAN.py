"""CFGAN on the HIP engine.

Reference: Dong-Kyu Chae et al., "CFGAN: A Generic Collaborative Filtering Framework based on Generative Adversarial
Networks." in CIKM 2018.
Plugin-compatible with model/general_recommender/CFGAN.py: same constructor, config keys (conf/CFGAN.properties: reg_G,
reg_D, lr_G, lr_D, ZR_ratio, ZP_ratio, ZR_coefficient, hiddenLayer_G, hiddenLayer_D, batchSize_G, batchSize_D, step_G,
step_D, mode, opt_G, opt_D, epochs, verbose), schedule, log lines (`metrics_info()` once, then `epoch %d:\\t%s` whenever
epoch % verbose == 0) and `evaluate()` / `predict(users, items)`.  The masks, both steps and the scorer are
neurec_amd/cfgan.py (csrc/cfgan.hip).

As the reference:
  * both masks hold the row's positives, and `g_zr_dims` is fed the whole zr row (CFGAN.py:137,171): the
    zero-reconstruction term pulls the outputs of the POSITIVES to 0 as well, not only those of the sampled negatives;
  * a row without a train entry is not in `user_pos_train`: its masks are empty, and it still sits in the batches (the
    iterators run over all rows), where it moves the biases and, through D, the kernels;
  * both regularisers take kernels AND biases (`get_collection(TRAINABLE_VARIABLES, scope=...)`);
  * `int(epochs / step_G)` outer epochs; per outer epoch new masks, then step_D passes over D's batches, then step_G
    passes over G's; each network has its own iterator (reshuffled per pass, the last short batch kept) and its own
    optimiser object, so two sets of Adam beta powers, each advanced on its own steps only.

Deviations, on purpose:
  * the masks come from the device's counter-based generator, not from numpy's `choice`: a row's sample at an outer epoch
    is a pure function of (seed, epoch, plane, row id), rebuilt when the row's batch comes up, so the D batch and the G
    batch of a row see the same masks without a [n_rows, n_cols] matrix;
  * the initial values come from numpy generators with fixed seeds (Xavier-uniform kernels in the creation order gen_h*,
    gen_out, dis_h*, dis_out; zero biases);
  * a sample size of 0 (a ratio of 0, or a row that holds almost every column) means no sample; the reference's
    `randint_choice` raises on it;
  * limits: 1 to 3 hidden layers of 1 to 512 units per network, batches up to 1,024 rows, opt_* in {adam, sgd}, mode in
    {userBased, itemBased}, ratios in [0, 1]; anything else is refused with the key and the range; multi-rank runs are
    refused;
  * predict() in full mode returns the [B, num_items] device tensor, in candidate mode per-user numpy arrays; no
    [n_rows, n_cols] rating matrix is kept.
"""
import numpy as np

from ...util import DataIterator
from .._common import require_single_gpu
from ..AbstractRecommender import AbstractRecommender


def initial_variables(n_cols, hidden_g, hidden_d, seed=2017):
    """{name: array} in the reference's creation order (CFGAN.py:97-123): Xavier-uniform kernels, zero biases"""
    rs = np.random.RandomState(seed)
    out = {}
    for net, widths, n_in, n_out in (("gen", hidden_g, n_cols, n_cols), ("dis", hidden_d, 2 * n_cols, 1)):
        dims = [int(n_in)] + [int(w) for w in widths] + [int(n_out)]
        for k in range(len(dims) - 1):
            name = "%s_h%d" % (net, k) if k < len(widths) else "%s_out" % net
            lim = np.sqrt(6.0 / (dims[k] + dims[k + 1]))
            out[name + "_kernel"] = rs.uniform(-lim, lim, (dims[k], dims[k + 1])).astype(np.float32)
            out[name + "_bias"] = np.zeros(dims[k + 1], np.float32)
    return out


class CFGAN(AbstractRecommender):
    def __init__(self, sess, dataset, conf):
        super(CFGAN, self).__init__(dataset, conf)
        self.dataset = dataset
        self.epochs = conf["epochs"]
        self.mode = conf["mode"]
        self.reg_G = conf["reg_G"]
        self.reg_D = conf["reg_D"]
        self.lr_G = conf["lr_G"]
        self.lr_D = conf["lr_D"]
        self.batchSize_G = conf["batchSize_G"]
        self.batchSize_D = conf["batchSize_D"]
        self.opt_g = conf["opt_G"]
        self.opt_d = conf["opt_D"]
        self.hiddenLayer_G = conf["hiddenLayer_G"]
        self.hiddenLayer_D = conf["hiddenLayer_D"]
        self.step_G = conf["step_G"]
        self.step_D = conf["step_D"]
        self.ZR_ratio = conf["ZR_ratio"]
        self.ZP_ratio = conf["ZP_ratio"]
        self.ZR_coefficient = conf["ZR_coefficient"]
        self.verbose = conf["verbose"]
        self.train_matrix = dataset.train_matrix.tocsr()
        # the model's rows: users, or items in itemBased mode (CFGAN.py:45-48 calls both num_users / num_items)
        self.num_rows, self.num_cols = self.train_matrix.shape[::-1] if self.mode == "itemBased" \
            else self.train_matrix.shape
        self.sess = sess                      # unused: there is no TensorFlow session
        self.engine = None

    def build_graph(self):
        from ...cfgan import CFGANEngine, check_config
        require_single_gpu("CFGAN")
        check_config(self.mode, self.hiddenLayer_G, self.hiddenLayer_D, self.batchSize_G, self.batchSize_D, self.opt_g,
                     self.opt_d, self.ZR_ratio, self.ZP_ratio)
        self.engine = CFGANEngine(initial_variables(self.num_cols, self.hiddenLayer_G, self.hiddenLayer_D),
                                  self.train_matrix, self.hiddenLayer_G, self.hiddenLayer_D, self.lr_G, self.lr_D,
                                  self.reg_G, self.reg_D, self.ZR_ratio, self.ZP_ratio, self.ZR_coefficient,
                                  self.batchSize_G, self.batchSize_D, opt_G=self.opt_g, opt_D=self.opt_d, mode=self.mode,
                                  seed=2018)

    def train_model(self):
        import torch
        engine = self.engine
        self.logger.info(self.evaluator.metrics_info())
        g_iter = DataIterator(np.arange(self.num_rows), batch_size=self.batchSize_G, shuffle=True, drop_last=False)
        d_iter = DataIterator(np.arange(self.num_rows), batch_size=self.batchSize_D, shuffle=True, drop_last=False)
        self.losses_d = torch.zeros((max(len(d_iter), 1), 3), device=engine.dev)
        self.losses_g = torch.zeros((max(len(g_iter), 1), 3), device=engine.dev)
        total_epochs = int(self.epochs / self.step_G)
        for epoch in range(total_epochs):
            engine.epoch = epoch                                  # new masks: a row's are rebuilt from (seed, epoch)
            for d_epoch in range(self.step_D):
                for n, idx in enumerate(d_iter):
                    engine.d_step(np.asarray(idx, dtype=np.int32), self.losses_d[n])
            for g_epoch in range(self.step_G):
                for n, idx in enumerate(g_iter):
                    engine.g_step(np.asarray(idx, dtype=np.int32), self.losses_g[n])
            if epoch % self.verbose == 0:
                self.logger.info("epoch %d:\t%s" % (epoch, self.evaluate()))

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
