"""One epoch of the reference's own data/sampler.py PairwiseSampler (compiled unchanged by oracle/Makefile,
oracle.ref.sampler_module()) on the toy train dict of tests/test_oracle_cpu.py::
test_reference_sampler_module_runs_an_epoch, batch by batch, written to tests/golden/ref_sampler_epoch.json.

    python tests/golden/make_ref_sampler_epoch.py          # needs oracle/_ref (make -C oracle ref)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TRAIN = {0: [1, 3], 2: [0], 5: [2, 4, 6, 7]}
N_ITEMS, BATCH = 10, 4


def epoch(mod):
    """[[users, pos, neg] per batch] of one unshuffled epoch, one negative per triplet"""
    class DS:
        num_items = N_ITEMS

        @staticmethod
        def get_user_train_dict():
            return TRAIN
    s = mod.PairwiseSampler(DS, neg_num=1, batch_size=BATCH, shuffle=False)
    return len(s), [[[int(x) for x in col] for col in b] for b in s]


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import ref
    mod = ref.sampler_module()
    assert mod is not None, "build oracle/_ref first: make -C oracle ref"
    n, batches = epoch(mod)
    with open(os.path.join(HERE, "ref_sampler_epoch.json"), "w") as f:
        json.dump({"len": n, "batches": batches}, f)
        f.write("\n")
    print("batches:", n)


if __name__ == "__main__":
    main()
