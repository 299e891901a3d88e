"""Generate tests/golden/svmwrite_golden.npz from the REAL reference on CPU: what the reference's own
``write_to_libsvm_without_masked`` (allrank/data/dataset_saving.py:9-32 -> scikit-learn's dump_svmlight_file) writes for small seeded
slates, byte for byte.  One case per feature count in ``FS`` (one-, two- and three-digit indices), each with 11 slates (two-digit
qids) handed over in the list form, ragged: slate s is ``x[s, :lens[s]]`` / ``y[s, :lens[s]]``, a numpy array or (``as_torch[s]``) a
torch tensor.  Every case holds: padding (y = -1) at slate ends, slate 1 padded from end to end (the reference then skips qid 1), an
all-zero kept row with label 2.5 in slate 0, -0.0 entries, non-integer labels, the edge values down the rows of slate 3 and along a
row of slate 4.  ``x`` [N, LMAX, F] / ``y`` [N, LMAX] are the same slates padded to one length: the [N, L, F] form of the same file.

    python tests/golden/make_golden_svmwrite.py        # build container only
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.ref_loader import load_reference  # noqa: E402

SEED = 920
FS = (1, 5, 20, 101)
LMAX = 24
LENS = [24, 5, 17, 16, 20, 9, 12, 1, 24, 7, 13]         # the list form's per-slate lengths
PADDED = [3, 5, 0, 2, 0, 1, 4, 0, 6, 0, 2]               # how many of them are padding, at the end
AS_TORCH = [0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0]
LABELS = np.asarray([0, 1, 2, 3, 4, 0.5, 2.5, 0.1, 1.75, 3.3], dtype=np.float32)
EDGE = np.asarray([0.1, 2.0 ** -24, 2.0 ** -23, 1e-45, 1.17549435e-38, 3.4028235e38, 1e15, 9.999999e15, 1e16, 1e-4, 9.99e-5, -2.5,
                   16777216, 123456.789], dtype=np.float32)


def case_inputs(F):
    rng = np.random.default_rng(SEED + F)
    n = len(LENS)
    x = rng.standard_normal((n, LMAX, F)).astype(np.float32)
    x[rng.random(x.shape) < (0.3 if F <= 20 else 0.85)] = 0.0       # (the widest case is sparse: the fixture stays small)
    x[rng.random(x.shape) < 0.05] = -0.0
    y = LABELS[rng.integers(0, len(LABELS), (n, LMAX))]
    for s, (k, p) in enumerate(zip(LENS, PADDED)):
        x[s, k - p:], y[s, k - p:] = 0.0, -1.0
    x[0, 1], y[0, 1] = 0.0, 2.5                          # "2.5 qid:0 \n"
    for i, v in enumerate(EDGE):                         # slate 3 keeps 14 rows
        x[3, i, i % F] = v
    x[4, 0, :min(F, len(EDGE))] = EDGE[:F]
    x[2, 0, 0], x[2, 0, F - 1] = 1.5, -3.25              # a row whose first and last columns are written
    return x, y


def slate_list(x, y, lens, as_torch):
    """the reference's argument form: per-slate arrays / tensors of their own lengths"""
    X = [torch.from_numpy(x[s, :k].copy()) if t else x[s, :k].copy() for s, (k, t) in enumerate(zip(lens, as_torch))]
    Y = [torch.from_numpy(y[s, :k].copy()) if t else y[s, :k].copy() for s, (k, t) in enumerate(zip(lens, as_torch))]
    return X, Y


def build():
    load_reference()
    from allrank.data.dataset_saving import write_to_libsvm_without_masked
    out = {"features": np.asarray(FS, dtype=np.int64), "lens": np.asarray(LENS, dtype=np.int64),
           "as_torch": np.asarray(AS_TORCH, dtype=np.uint8)}
    for F in FS:
        x, y = case_inputs(F)
        X, Y = slate_list(x, y, LENS, AS_TORCH)
        fd, path = tempfile.mkstemp(suffix=".svm")
        os.close(fd)
        try:
            write_to_libsvm_without_masked(path, X, Y)
            text = np.fromfile(path, dtype=np.uint8)
        finally:
            os.remove(path)
        assert b"qid:0 " in text.tobytes() and b"qid:1 " not in text.tobytes() and b"\n2.5 qid:0 \n" in text.tobytes()
        out["F%d.x" % F], out["F%d.y" % F], out["F%d.text" % F] = x, y, text
    return {"svmwrite_golden.npz": out}


def main():
    for f, d in build().items():
        np.savez_compressed(os.path.join(HERE, f), **d)
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
