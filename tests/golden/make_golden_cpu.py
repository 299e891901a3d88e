"""Generate tests/golden/cpu_golden.npz from the REAL reference (CPU, where a checkout of allegro/allRank is present):
    python tests/golden/make_golden_cpu.py
The reference's answers on the seeded inputs of three CPU tests, so that those tests run without the reference:
  * ``model.<i>.*``  -- tests/test_model_cpu.py::test_same_seed_gives_reference_initial_weights: the reference's make_model
    (allrank/models/model.py:131-151) under torch.manual_seed(42) for the i-th config of that test: state_dict entries in order,
    parameter names in order, and for a positional encoding the position module's output on a fixed input;
  * ``fixlength.*``  -- tests/test_data_cpu.py::test_against_reference_fixlength_pad_and_libsvm_roundtrip: FixLength + ToTensor
    (dataset_loading.py:19-93) of every slate of the test's toy data set;
  * ``loader<L>.*``  -- tests/test_loader_cpu.py::test_oracle_loader_equals_the_reference_loader: every batch of the loader traffic of
    two epochs of the reference's create_data_loaders / load_libsvm_dataset (dataset_loading.py:197-248) under main.py:36-38's seeds.
"""
import copy
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.ref_loader import load_reference  # noqa: E402


def _loader(out):
    import pathlib
    from tests import test_loader_cpu as T
    import allrank.data.dataset_loading as RD
    for L in T.LOADER_SLATE_LENGTHS:
        with tempfile.TemporaryDirectory() as tmp:
            path = T._write(pathlib.Path(tmp), long={3: 33, 8: 12})
            T._seed()
            batches = T._epochs(*RD.create_data_loaders(*RD.load_libsvm_dataset(path, L, "vali"), num_workers=0, batch_size=8))
        out["loader%d.n" % L] = np.int64(len(batches))
        for j, b in enumerate(batches):
            for name, t in zip("xyi", b):
                out["loader%d.%d.%s" % (L, j, name)] = t.numpy()


def _fixlength(out):
    from tests import test_data_cpu as T
    from allrank.data.dataset_loading import FixLength, ToTensor
    X, y, qid, lens = T._toy(seed=4, n_q=12)
    off = np.concatenate([[0], np.cumsum(lens)])
    fl, tt = FixLength(T.FIXLENGTH_L), ToTensor()
    for s in range(12):
        rx, ry, ri = tt(fl((X[off[s]:off[s + 1]].astype(np.float64), y[off[s]:off[s + 1]], None)))
        out["fixlength.%d.x" % s], out["fixlength.%d.y" % s], out["fixlength.%d.i" % s] = rx.numpy(), ry.numpy(), ri.numpy()


def _model(out):
    from tests import test_model_cpu as T
    from allrank.models.model import make_model as ref_make
    from allrank.config import TransformerConfig, PositionalEncoding
    for i, kw in enumerate(T.SEED_CONFIGS):
        k1 = copy.deepcopy(kw)
        if k1["transformer"]:
            if k1["transformer"]["positional_encoding"]:
                k1["transformer"]["positional_encoding"] = PositionalEncoding(**k1["transformer"]["positional_encoding"])
            k1["transformer"] = TransformerConfig(**k1["transformer"])
        torch.manual_seed(42)
        ref = ref_make(**k1)
        sd = ref.state_dict()
        out["model.%d.keys" % i] = np.asarray(list(sd.keys()))
        out["model.%d.params" % i] = np.asarray([n for n, _ in ref.named_parameters()])
        for j, v in enumerate(sd.values()):
            out["model.%d.sd.%d" % (i, j)] = v.numpy()
        if kw["transformer"] and kw["transformer"]["positional_encoding"]:
            x, idx = T.position_inputs(kw)
            out["model.%d.pos_x" % i] = x.numpy()
            out["model.%d.pos_out" % i] = ref.encoder.position(x, idx == -1, idx.clone()).detach().numpy()


def build():
    out = {}
    load_reference(stable_sort=False)
    _loader(out)
    _fixlength(out)
    load_reference()
    _model(out)
    return {"cpu_golden.npz": out}


def main():
    for f, d in build().items():
        np.savez_compressed(os.path.join(HERE, f), **d)
        print("wrote", f, len(d), "arrays")


if __name__ == "__main__":
    main()
