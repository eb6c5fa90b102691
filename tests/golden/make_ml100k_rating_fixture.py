"""The reference's real ml-100k ratings (dataset/ml-100k.rating: 100,000 `user<TAB>item<TAB>rating<TAB>time` lines,
the file the default NeuRec.properties reads) as a compact fixture: tests/golden/ml100k_rating.npz, the four
columns in file order.  `write_rating_file` writes the same text back for the Dataset tests.

    python tests/golden/make_ml100k_rating_fixture.py       # needs the reference tree (oracle/ref_models.REF)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "ml100k_rating.npz")


def write_rating_file(path, fixture=FIXTURE):
    """the rating file as the reference tree holds it, from the fixture"""
    z = np.load(fixture)
    cols = np.stack([z["user"], z["item"], z["rating"], z["time"]], axis=1).astype(np.int64)
    with open(path, "w") as f:
        f.write("".join("%d\t%d\t%d\t%d\n" % tuple(r) for r in cols.tolist()))
    return path


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle.ref_models import REF
    SRC = os.path.join(REF, "dataset", "ml-100k.rating")
    a = np.loadtxt(SRC, delimiter="\t", dtype=np.int64)
    assert a.shape == (100000, 4)
    np.savez_compressed(FIXTURE, user=a[:, 0].astype(np.int16), item=a[:, 1].astype(np.int16),
                        rating=a[:, 2].astype(np.int8), time=a[:, 3].astype(np.int32))
    tmp = FIXTURE + ".check"
    write_rating_file(tmp)
    with open(tmp, "rb") as f, open(SRC, "rb") as g:
        assert f.read() == g.read(), "the fixture does not give the file back byte for byte"
    os.remove(tmp)
    print("ratings:", len(a), "fixture bytes:", os.path.getsize(FIXTURE))


if __name__ == "__main__":
    main()
