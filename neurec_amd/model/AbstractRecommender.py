"""AbstractRecommender — the plugin base class (model/AbstractRecommender.py:23-45).

Subclasses live in `model/<family>_recommender/<Name>.py`, take `(sess, dataset, conf)` (the
first argument was the TensorFlow session; it is accepted and ignored), and implement
`build_graph()`, `train_model()` and `predict(user_ids, candidate_items)`.  The constructor
builds the evaluator and the logger exactly as the reference does, so log paths, the dataset /
config dump and the metric header are unchanged.
"""
import os
import time

from ..evaluator import ProxyEvaluator
from ..util.logger import Logger


def _create_logger(config, data_name):
    """log/<dataset>/<model>/<dataset>_<params[:150]>_<timestamp>.log (AbstractRecommender.py:9-20)."""
    param_str = "%s_%s" % (data_name, config.params_str())
    run_id = "%s_%.8f" % (param_str[:150], time.time())
    log_dir = os.path.join("log", data_name, config["recommender"])
    return Logger(os.path.join(log_dir, run_id + ".log"))


class _Silent(object):
    """the logger of ranks > 0 of a multi-GPU run"""
    def __getattr__(self, name):
        return lambda *a, **k: None


class AbstractRecommender(object):
    def __init__(self, dataset, conf):
        self.evaluator = ProxyEvaluator(dataset.get_user_train_dict(),
                                        dataset.get_user_test_dict(),
                                        dataset.get_user_test_neg_dict(),
                                        metric=conf["metric"],
                                        group_view=conf["group_view"],
                                        top_k=conf["topk"],
                                        batch_size=conf["test_batch_size"],
                                        num_thread=conf["num_thread"])
        # one rank of several (parallel.get_comm): rank 0 writes the run's log, the others only compute
        rank = int(os.environ.get("RANK", "0")) if int(os.environ.get("WORLD_SIZE", "1")) > 1 else 0
        self.logger = _create_logger(conf, dataset.dataset_name) if rank == 0 else _Silent()
        self.logger.info(dataset)
        self.logger.info(conf)

    def build_graph(self):
        raise NotImplementedError

    def train_model(self):
        raise NotImplementedError

    def predict(self, user_ids, items):
        raise NotImplementedError


class SeqAbstractRecommender(AbstractRecommender):
    """base of `model/sequential_recommender/` (AbstractRecommender.py:48-52): the dataset must carry timestamps"""
    def __init__(self, dataset, conf):
        if dataset.time_matrix is None:
            raise ValueError("Dataset does not contant time infomation!")
        super(SeqAbstractRecommender, self).__init__(dataset, conf)


def read_trust_lines(path, sep, userids):
    """the (user row, friend row) pairs of a trust file with two columns, in file order: lines whose user or friend is
    no key of `userids` are dropped (AbstractRecommender.py:58-70).  Deviation, on purpose: the file's columns and the
    keys are compared in their STRING form — the reference's np.in1d keeps nothing when the file parses as integers
    and the keys are strings (or the other way round)"""
    import pandas as pd
    lines = pd.read_csv(path, sep=sep, header=None, names=["user", "friend"], dtype=str, skipinitialspace=True)
    by_text = {str(k).strip(): int(v) for k, v in userids.items()}
    user = lines["user"].astype(str).str.strip().map(by_text)
    friend = lines["friend"].astype(str).str.strip().map(by_text)
    keep = user.notna() & friend.notna()
    return user[keep].astype("int64").to_numpy(), friend[keep].astype("int64").to_numpy()


class SocialAbstractRecommender(AbstractRecommender):
    """base of `model/social_recommender/` (AbstractRecommender.py:55-73): `social_matrix` [U, U], the directed trust
    matrix of conf["social_file"] as given — row = the user, column = the user they trust; duplicate lines collapse to
    one index"""
    def __init__(self, dataset, conf):
        import scipy.sparse as sp
        super(SocialAbstractRecommender, self).__init__(dataset, conf)
        user_id, friend_id = read_trust_lines(conf["social_file"], conf["data.convert.separator"], dataset.userids)
        num_users, num_items = dataset.train_matrix.shape
        self.social_matrix = sp.csr_matrix(([1] * len(user_id), (user_id, friend_id)), shape=(num_users, num_users))
