"""-m gpu: END-TO-END parity with the reference's own training run on a job whose training slates are SAMPLED (FixLength's sampling
branch, dataset_loading.py:61-79) -- the case tests/test_gpu_trajectory.py's jobs leave out.

tests/golden/trajectory_sampled_golden.npz holds what ``allrank.main.run()`` produced on CPU on one ragged attention + ApproxNDCG job
(slate_length 32 under slates of up to 48 items, six single-relevant long slates, validation slates longer than the training slate
length; generator: tests/golden/make_golden_trajectory_sampled.py), once with ``num_workers`` 1 and once with 0.  Here the same job
runs through ``load_libsvm_dataset`` -> ``DeviceLoader(sampling="reference", num_workers=W)`` -> ``allrank_amd.fit.fit``:

  * the ``indices`` of every training batch of every epoch are IDENTICAL to the reference's (the same draws, fit() burning or making
    the reference's extra passes in step);
  * losses, metrics and the weights after every epoch stay within the drift bounds of tests/test_gpu_trajectory.py.
"""
import json
import os
import types
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

# copied from tests/test_gpu_trajectory.py (BOUNDS; measured there, profiles/r06_trajectory_drift.md): relative to 1 + |reference value|;
# weights absolute
BOUNDS = {"train_loss_epoch0": 1e-5, "train_loss": 5e-5, "val_loss": 5e-5, "metric": 1e-3, "weights_max": 4e-3, "weights_rms": 1e-4}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "trajectory_sampled_golden.npz"), allow_pickle=False)


def _run(golden, W, tmp_path, train_metrics):
    from torch import optim
    from tests.golden.make_golden_trajectory import write_job_files
    from allrank_amd import data as ED, fit as EF, losses
    from allrank_amd.engine import FusedTrainer
    from allrank_amd.model import make_model
    cfg = json.loads(str(golden["w%d/config" % W]))
    data = {role: tuple(golden["data/%s/%s" % (role, k)] for k in ("X", "y", "qid")) for role in ("train", "vali")}
    folder = str(tmp_path / "job")
    write_job_files(data, folder)
    torch.manual_seed(42)                                            # main.py:36-38
    torch.cuda.manual_seed_all(42)
    np.random.seed(42)
    tr_ds, va_ds = ED.load_libsvm_dataset(folder, cfg["data"]["slate_length"], cfg["data"]["validation_ds_role"], device=DEV)
    n_features = tr_ds.shape[-1]
    bs = cfg["data"]["batch_size"]
    tr = ED.DeviceLoader(tr_ds, bs, shuffle=True, sampling="reference", num_workers=W)
    va = ED.DeviceLoader(va_ds, bs, shuffle=False, sampling="reference", num_workers=W)
    model = make_model(n_features=n_features, **json.loads(json.dumps(cfg["model"])))
    model.to(DEV)
    init = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    optimizer = getattr(optim, cfg["optimizer"]["name"])(params=model.parameters(), **cfg["optimizer"]["args"])
    loss_func = partial(getattr(losses, cfg["loss"]["name"]), **cfg["loss"]["args"])
    metrics = {}
    for m in cfg["metrics"]:
        n, at = m.split("_")
        metrics.setdefault(n, []).append(int(at))
    config = types.SimpleNamespace(metrics=metrics, val_metric=cfg["val_metric"], detect_anomaly=False)
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    epochs, indices, cur, hist = [], [], [], []
    orig_info, orig_step = EF.log.info, FusedTrainer.step

    def step(self, xb, yb, indices=None, global_batch=None, lengths=None):
        cur.append(indices[:int(global_batch)].cpu().numpy())
        return orig_step(self, xb, yb, indices, global_batch=global_batch, lengths=lengths)

    def spy(msg, *a):
        if isinstance(msg, str) and msg.startswith("Epoch :"):
            def parse(s_):
                t = s_.split()
                return {t[i + 1]: float(t[i + 2]) for i in range(0, len(t), 3)} if t else {}
            hist.append((parse(a[3]), parse(a[4])))
            epochs.append(dict(train_loss=float(a[1]), val_loss=float(a[2]),
                               weights={k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}))
            indices.append(list(cur))
            del cur[:]
        return orig_info(msg, *a)
    EF.log.info, FusedTrainer.step = spy, step
    try:
        EF.fit(model=model, loss_func=loss_func, optimizer=optimizer, scheduler=None, train_dl=tr, valid_dl=va, config=config,
               device=torch.device(DEV), output_dir=str(out), tensorboard_output_path=None, train_metrics=train_metrics, **cfg["training"])
    finally:
        EF.log.info, FusedTrainer.step = orig_info, orig_step
    return dict(cfg=cfg, init=init, epochs=epochs, indices=indices, hist=hist, run=dict(EF.last_run))


@pytest.mark.parametrize("train_metrics", [None, "reference"])
@pytest.mark.parametrize("W", [1, 0])
def test_sampled_fit_trajectory_equals_the_reference_run(golden, tmp_path, W, train_metrics):
    got = _run(golden, W, tmp_path, train_metrics)
    p = "w%d/" % W
    names = [str(m) for m in golden["metric_names"]]
    E = len(golden[p + "train_loss"])
    assert got["run"]["engine"] == "fused" and got["run"]["sampling"] == "reference", got["run"]
    assert len(got["epochs"]) == E
    for k, v in got["init"].items():
        assert np.array_equal(v, golden["init/" + k]), ("initial weights", k)
    # the reference's draws: the same items in the same slots of the same batches, every epoch
    sampled = 0
    for e in range(E):
        assert [len(b) for b in got["indices"][e]] == golden[p + "batch_sizes_epoch%d" % e].tolist(), ("batch sizes", e)
        mine = np.concatenate(got["indices"][e])
        assert np.array_equal(mine, golden[p + "indices_epoch%d" % e].astype(np.int64)), ("indices", e)
        sampled += int(((mine >= 0).all(1) & (mine != np.arange(mine.shape[1])).any(1)).sum())
    assert sampled > 0
    rel = lambda a, b: abs(a - b) / (1.0 + abs(b))  # noqa: E731
    d_train = [rel(got["epochs"][e]["train_loss"], float(golden[p + "train_loss"][e])) for e in range(E)]
    d_val = [rel(got["epochs"][e]["val_loss"], float(golden[p + "val_loss"][e])) for e in range(E)]
    d_vm = [[abs(got["hist"][e][1][m] - float(golden[p + "val_metrics"][e][j])) for j, m in enumerate(names)] for e in range(E)]
    d_tm = [[abs(got["hist"][e][0][m] - float(golden[p + "train_metrics"][e][j])) for j, m in enumerate(names)] for e in range(E)]
    # parameters the loss does not depend on random-walk in both runs (tests/test_gpu_trajectory.py): output bias, the final
    # LayerNorm's bias, every layer's key-projection bias
    free = ["output_layer.w_1.bias", "encoder.norm.b_2"] + ["encoder.layers.%d.self_attn.linears.1.bias" % i
                                                            for i in range(got["cfg"]["model"]["transformer"]["N"])]
    wmax, wrms = [], []
    for e in range(E):
        d = np.concatenate([(got["epochs"][e]["weights"][k].astype(np.float64) - golden["%sweights_epoch%d/%s" % (p, e, k)]).ravel()
                            for k in got["init"] if k not in free])
        wmax.append(float(np.abs(d).max()))
        wrms.append(float(np.sqrt((d ** 2).mean())))
    drift = dict(W=W, train_metrics=train_metrics or "fused", train_loss=d_train, val_loss=d_val, val_metrics=d_vm,
                 train_metrics_drift=d_tm if train_metrics == "reference" else None, weights_max=wmax, weights_rms=wrms)
    print("sampled trajectory drift:", json.dumps(drift))
    assert d_train[0] <= BOUNDS["train_loss_epoch0"], d_train
    assert max(d_train) <= BOUNDS["train_loss"] and max(d_val) <= BOUNDS["val_loss"], (d_train, d_val)
    assert max(max(r) for r in d_vm) <= BOUNDS["metric"], d_vm
    if train_metrics == "reference":                        # (the default takes the train metrics from the training forward instead)
        assert max(max(r) for r in d_tm) <= BOUNDS["metric"], d_tm
    assert max(wmax) <= BOUNDS["weights_max"] and max(wrms) <= BOUNDS["weights_rms"], (wmax, wrms)
