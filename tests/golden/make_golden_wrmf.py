"""Golden WRMF trace produced by the REFERENCE's own WRMF class (model/general_recommender/WRMF.py).

The class is imported whole and unchanged through oracle/ref_models.py and runs under oracle/tf_shim.py, as
make_golden_tfgraph.py does for MF / LightGCN / NGCF / MultiVAE.  WRMF uses three TensorFlow calls the shim does not
carry — `tf.eye`, `tf.linalg.solve` and `tf.scatter_update` — so this file attaches them to the shim module before the
class is loaded (their published definitions: the identity matrix; the solution of A X = B by LU with partial
pivoting, torch.linalg.solve = LAPACK gesv, as TF's MatrixSolveOp; a row overwrite of the variable applied when the
op is run, like the shim's `assign`).  Everything else — the dense Cui / Pui matrices, YTY + YTCuIY + lambda I, the
per-user then per-item `sess.run` loops of train_model(), evaluate()'s `sess.run([user_embeddings, item_embeddings])`
and predict() — is the reference's code executing.

    python tests/golden/make_golden_wrmf.py              # needs /root/reference

Writes tests/golden/tfgraph_wrmf.npz: the train pattern (indptr / indices / shape), the initial tables P0 / Q0, the
hyper-parameters, and for each float width (`f32_*`, `f64_*`, the f64 twin from the same P0 / Q0) the tables after
every epoch (`P` / `Q`: [epochs, rows, d]) and the score rows predict() returned at every epoch's evaluation for the
users `ratings_users` (`ratings`: [epochs, users, items]).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_models as rm          # noqa: E402
from oracle import tf_shim                    # noqa: E402
from make_golden_tfgraph import WIDTHS, _np, _reset_recorders, toy_matrix   # noqa: E402

HYPER = dict(embedding_size=16, alpha=10.0, topk=20, epochs=2, reg_mf=0.1, init_method="uniform", stddev=0.01,
             verbose=1)


# ------------------------------------------------------------------ the three ops WRMF needs on top of the shim
def _eye(num_rows, num_columns=None, dtype=None, name=None):
    return tf_shim._Const(torch.eye(num_rows, num_columns or num_rows, dtype=tf_shim.float_dtype()))


def _solve(matrix, rhs, adjoint=False, name=None):
    assert not adjoint
    return tf_shim.Tensor(lambda a, b: torch.linalg.solve(a, b), [matrix, rhs])


def _scatter_update(ref, indices, updates, use_locking=True, name=None):
    op = tf_shim._Op()
    op.tensors = [indices, updates]

    def prepare(sess, values):
        op._rows = values[0].reshape(-1).to(torch.int64).clone()
        op._new = values[1].detach().clone()

    def apply(sess):
        ref.value[op._rows] = op._new.to(ref.value.dtype)
    op.prepare, op.apply = prepare, apply
    return op


def attach_ops():
    tf_shim.eye = _eye
    tf_shim.linalg = types.SimpleNamespace(solve=_solve)
    tf_shim.scatter_update = _scatter_update


# ------------------------------------------------------------------ the run
def run_wrmf(R, P0, Q0, hyper, ratings_users):
    out = {}
    tables = []
    evaluate = rm.RecordingEvaluator.evaluate

    def recording(self, model):
        # WRMF.evaluate fetched the tables with sess.run([user_embeddings, item_embeddings]) just before
        tables.append((np.array(model._cur_user_embeddings), np.array(model._cur_item_embeddings)))
        return evaluate(self, model)

    rm.RecordingEvaluator.evaluate = recording
    try:
        for tag, width in WIDTHS:
            _reset_recorders()
            del tables[:]
            rm.RecordingEvaluator.users = ratings_users
            model, sess, _ = rm.build("WRMF", rm.Dataset(R), hyper, width)
            model.user_embeddings.load(P0)
            model.item_embeddings.load(Q0)
            model.train_model()
            assert len(tables) == hyper["epochs"]
            out[tag + "_P"] = _np(np.stack([t[0] for t in tables]), width)
            out[tag + "_Q"] = _np(np.stack([t[1] for t in tables]), width)
            out[tag + "_ratings"] = _np(np.stack(rm.RecordingEvaluator.ratings), width)
            out[tag + "_log_lines"] = np.asarray([ln for ln in rm.MemoryLogger.lines if ln.startswith("iteration")])
    finally:
        rm.RecordingEvaluator.evaluate = evaluate
    return out


def main():
    if not rm.available():
        raise SystemExit("needs the reference tree (%s)" % rm.REF)
    attach_ops()
    R = toy_matrix()
    U, I = R.shape
    d = HYPER["embedding_size"]
    rs = np.random.RandomState(77)
    P0 = rs.uniform(-0.5, 0.5, (U, d)).astype(np.float32)
    Q0 = rs.uniform(-0.5, 0.5, (I, d)).astype(np.float32)
    users = np.arange(0, U, 15, dtype=np.int32)
    out = run_wrmf(R, P0, Q0, HYPER, users.tolist())
    out.update(indptr=R.indptr.astype(np.int64), indices=R.indices.astype(np.int32),
               shape=np.asarray(R.shape, np.int64), P0=P0, Q0=Q0, ratings_users=users,
               alpha=np.float64(HYPER["alpha"]), reg_mf=np.float64(HYPER["reg_mf"]),
               epochs=np.int64(HYPER["epochs"]))
    path = os.path.join(HERE, "tfgraph_wrmf.npz")
    np.savez_compressed(path, **out)
    gap = max(np.abs(out["f32_%s" % t] - out["f64_%s" % t]).max() for t in "PQ")
    print("wrote %s (%d bytes); fp32 vs fp64 trace gap %.3g" % (path, os.path.getsize(path), gap))


if __name__ == "__main__":
    main()
