"""-m gpu: a 46-feature libsvm job (the feature count of MQ2007 / MQ2008) through fit(): the fused step is taken -- it used to die in
its first batch -- from the host loader and from the device-resident loader, and the run agrees with the autograd Trainer's
(``use_fused=False``) at the bars tests/test_gpu_fit.py holds that comparison to: training ndcg_5 within 2e-3, validation ndcg_5
within 5e-3.  Two epochs of three batches (one of them short), no shuffling and no dropout, so both engines see the same steps."""
import copy
import types
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F, L_TRAIN, BS = 46, 30, 16


def _write(tmp_path):
    import bench
    rng = np.random.default_rng(9)
    for role, n in (("train", 40), ("vali", 27)):
        lens = np.clip(rng.integers(1, 45 if role == "vali" else L_TRAIN + 1, n), 1, None)
        bench.write_synth_libsvm(str(tmp_path / ("%s.txt" % role)), lens, F, 5 if role == "train" else 6)


def _loaders(kind, tmp_path):
    """the two files as resident sets behind DeviceLoaders, or as the padded host tensors of a torch DataLoader (the same slates in
    the same order: every training slate fits the slate length, so nothing is sampled)"""
    from torch.utils.data import DataLoader, TensorDataset
    from allrank_amd import data as ED
    tr, va = ED.load_libsvm_dataset(str(tmp_path), L_TRAIN, "vali", device=DEV)
    assert tr.slates.n_features == F and va.slate_length > L_TRAIN
    if kind == "resident":
        return ED.DeviceLoader(tr, BS, shuffle=False), ED.DeviceLoader(va, BS, shuffle=False)
    out = []
    for ds in (tr, va):
        ids = torch.arange(len(ds), dtype=torch.int64, device=DEV)
        out.append(DataLoader(TensorDataset(*[t.cpu() for t in ds.slates.batch(ids, ds.slate_length, seed=0)]), batch_size=BS, shuffle=False))
    return out[0], out[1]


def _fit(kind, tmp_path, use_fused, val_scorer=None):
    from allrank_amd import fit as EF, losses as E
    from tests.test_gpu_fit import _model
    train_dl, val_dl = _loaders(kind, tmp_path)
    model = _model(F)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    cfg = types.SimpleNamespace(metrics={"ndcg": [5]}, val_metric="ndcg_5")
    res = EF.fit(epochs=2, model=model, loss_func=partial(E.approxNDCGLoss), optimizer=opt, scheduler=None, train_dl=train_dl,
                 valid_dl=val_dl, config=cfg, gradient_clipping_norm=None, early_stopping_patience=5, device=torch.device(DEV),
                 output_dir=str(tmp_path), tensorboard_output_path=None, use_fused=use_fused, compact=False, val_scorer=val_scorer)
    assert tuple(model.input_layer.layers[0].weight.shape) == (32, F)
    return res, copy.deepcopy(EF.last_run)


@pytest.mark.parametrize("kind", ["host", "resident"])
def test_fit_takes_the_fused_step_at_46_features(kind, tmp_path):
    _write(tmp_path)
    res_f, run_f = _fit(kind, tmp_path, True)
    assert run_f["engine"] == "fused" and not run_f["fcstep"], run_f
    res_a, run_a = _fit(kind, tmp_path, False)
    assert run_a["engine"] == "autograd"
    res_p, run_p = _fit(kind, tmp_path, True, val_scorer="packed")
    assert run_p["engine"] == "fused" and run_p["val_scorer"] == "packed" and run_p["val_scorer_reason"] == "", run_p
    d_train = abs(float(res_f["train_metrics"]["ndcg_5"]) - float(res_a["train_metrics"]["ndcg_5"]))
    d_val = abs(float(res_f["val_metrics"]["ndcg_5"]) - float(res_a["val_metrics"]["ndcg_5"]))
    d_packed = abs(float(res_p["val_metrics"]["ndcg_5"]) - float(res_f["val_metrics"]["ndcg_5"]))
    print("%s: fused %r autograd %r packed %r" % (kind, res_f, res_a, res_p))
    assert len(run_f["epoch_log"]) == len(run_a["epoch_log"]) == len(run_p["epoch_log"]) == 2
    assert all(np.isfinite(e["val_loss"]) for e in run_f["epoch_log"] + run_p["epoch_log"])
    assert d_train < 2e-3 and d_val < 5e-3, (res_f, res_a)
    assert d_packed <= 1e-5, (res_p, res_f)                # (the packed scorer against the module scorer: tests/test_gpu_packed_scorer.py's bar)
    for e_p, e_f in zip(run_p["epoch_log"], run_f["epoch_log"]):
        assert abs(e_p["val_loss"] - e_f["val_loss"]) <= 1e-6 * max(1.0, abs(e_f["val_loss"])), (e_p, e_f)
