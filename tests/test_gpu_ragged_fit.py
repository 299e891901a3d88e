"""-m gpu: fit(val_scorer="ragged") -- the packed scorer with the validation loss and metrics on the packed rows (allrank_amd.ragged)
-- against fit(val_scorer="packed") on the small job of tests/test_gpu_packed_scorer.py (validation slates up to 5x the training
length), at that file's bars: validation loss 1e-6 relative, NDCG 1e-5."""
from functools import partial

import pytest
import torch

from tests.test_gpu_packed_scorer import _device_loaders, _fit, _host_loaders

pytestmark = pytest.mark.gpu


def _same_run(a, b):
    (res_a, run_a), (res_b, run_b) = a, b
    assert len(run_a["epoch_log"]) == len(run_b["epoch_log"]) == 2
    for e_a, e_b in zip(run_a["epoch_log"], run_b["epoch_log"]):
        print("val_loss ragged", e_a["val_loss"], "packed", e_b["val_loss"])
        assert abs(e_a["val_loss"] - e_b["val_loss"]) <= 1e-6 * max(1.0, abs(e_b["val_loss"])), (e_a, e_b)
    for k in ("ndcg_5", "ndcg_10"):
        print(k, "ragged", float(res_a["val_metrics"][k]), "packed", float(res_b["val_metrics"][k]))
        assert abs(float(res_a["val_metrics"][k]) - float(res_b["val_metrics"][k])) <= 1e-5, k


@pytest.mark.parametrize("kind", ["host", "resident"])
def test_fit_ragged_matches_packed_with_approxndcg(kind, tmp_path, monkeypatch):
    from allrank_amd import losses as E

    def loaders():
        return _host_loaders() if kind == "host" else _device_loaders(tmp_path)
    loss = partial(E.approxNDCGLoss, alpha=1.5)
    packed = _fit("packed", tmp_path, loaders(), loss=loss)
    ragged = _fit("ragged", tmp_path, loaders(), loss=loss)
    assert packed[1]["val_scorer"] == "packed" and "val_eval" not in packed[1]
    assert ragged[1]["val_scorer"] == "ragged" and ragged[1]["val_scorer_reason"] == ""
    assert ragged[1]["val_eval"] == {"loss": "ragged", "metrics": "ragged"}
    _same_run(ragged, packed)
    if kind == "host":                                     # the environment variable does the same under main.py
        env = _fit(None, tmp_path, loaders(), loss=loss, env="ragged", monkeypatch=monkeypatch)
        assert env[1]["val_scorer"] == "ragged" and env[1]["val_eval"] == ragged[1]["val_eval"]
        assert [e["val_loss"] for e in env[1]["epoch_log"]] == [e["val_loss"] for e in ragged[1]["epoch_log"]]


def test_fit_ragged_with_lambdaloss_mean_keeps_the_batch_global_pair_count(tmp_path):
    from allrank_amd import losses as E
    loss = partial(E.lambdaLoss, weighing_scheme="ndcgLoss2PP_scheme", k=10, reduction="mean")
    ragged = _fit("ragged", tmp_path, _host_loaders(), loss=loss)
    assert ragged[1]["val_eval"] == {"loss": "ragged", "metrics": "ragged"}
    _same_run(ragged, _fit("packed", tmp_path, _host_loaders(), loss=loss))


def test_fit_ragged_keeps_listmle_on_the_padded_grid(tmp_path):
    """listMLE has no ragged form (its column shuffle is defined over padded columns): the loss runs as under "packed", the metrics
    ragged.  The loss draws its shuffle from torch's global generator in both runs, seeded alike by ``_fit``."""
    from allrank_amd import losses as E
    loss = partial(E.listMLE)
    ragged = _fit("ragged", tmp_path, _host_loaders(), loss=loss)
    assert ragged[1]["val_scorer"] == "ragged" and ragged[1]["val_eval"] == {"loss": "padded", "metrics": "ragged"}
    _same_run(ragged, _fit("packed", tmp_path, _host_loaders(), loss=loss))


def test_fit_ragged_reports_the_module_path_for_stochastic_neuralndcg(tmp_path):
    from allrank_amd import losses as E
    res, run = _fit("ragged", tmp_path, _host_loaders(), loss=partial(E.neuralNDCG, stochastic=True), epochs=1)
    assert run["val_scorer"] == "module" and "stochastic" in run["val_scorer_reason"] and "val_eval" not in run


def test_scorer_packed_is_the_grid_without_its_padding():
    """FusedScorer.packed(): scores and labels of the valid slots of scores_raw / y in slate order, cu / order / max_len of the batch --
    from host lengths and from device-counted ones"""
    from allrank_amd.engine import FusedTrainer
    from tests.test_gpu_packed_scorer import _model, _ragged
    model = _model(24)
    ft = FusedTrainer(model, "listNet", {}, 4, 40, lr=1e-3, use_graph=True)
    lens = [60, 1, 0, 44, 59]
    x, y, idx, hl = _ragged(lens, 60, 24, 5)
    sc_ = ft.scorer(6, 60)                                 # one more slate than the batch: topped up with an empty one
    for lengths in (hl, None):
        grid = sc_.run(x, y, idx, lengths=lengths).clone()
        s_p, y_p, cu, order, max_len = sc_.packed()
        valid = sc_.y != -1
        assert max_len == 60 and cu.tolist() == [0, 60, 61, 61, 105, 164, 164] and s_p.shape == y_p.shape == (164,)
        assert torch.equal(s_p, grid[valid]) and torch.equal(y_p, sc_.y[valid])
        assert sorted(order.tolist()) == list(range(6)) and order.tolist()[:2] == [0, 4]
