"""The reference's own compiled evaluator (oracle/_ref) on the seeded inputs of
tests/test_oracle_cpu.py::test_oracle_equals_live_reference_on_fresh_inputs: its eval_matrix and arg_topk
results per trial, written to tests/golden/ref_fresh_inputs.npz (the inputs are regenerated from the seed).

    python tests/golden/make_golden_fresh_inputs.py        # needs oracle/_ref (make -C oracle ref)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
METRICS = [1, 2, 3, 4, 5]


def fresh_inputs():
    """12 (scores, truth, k) trials: plain, coarsely rounded (ties) and partly -inf score rows"""
    rng = np.random.RandomState(7)
    for trial in range(12):
        rows, cols = 40, int(rng.randint(60, 2500))
        k = int(rng.randint(1, min(60, cols // 2)))
        s = rng.randn(rows, cols).astype(np.float32)
        if trial % 3 == 1:
            s = (np.round(s * 3) / 3).astype(np.float32)
        if trial % 3 == 2:
            s[rng.rand(rows, cols) < 0.3] = -np.inf
        truth = [np.sort(rng.choice(cols, rng.randint(1, 30), replace=False)).tolist()
                 for _ in range(rows)]
        yield s, truth, k


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import ref
    assert ref.available(), "build oracle/_ref first: make -C oracle ref"
    out = {}
    for t, (s, truth, k) in enumerate(fresh_inputs()):
        out["eval_%d" % t] = ref.eval_matrix(s.copy(), truth, METRICS, k)
        out["topk_%d" % t] = ref.arg_topk(s.copy(), k)
    np.savez_compressed(os.path.join(HERE, "ref_fresh_inputs.npz"), **out)
    print("trials:", len(out) // 2, "bytes:", os.path.getsize(os.path.join(HERE, "ref_fresh_inputs.npz")))


if __name__ == "__main__":
    main()
