"""-m gpu: FusedTrainer(narrow_heads=True) -- the split-bf16 attention forward for head widths up to 32 (ltrx_mha_fwd_narrow) behind
the training forward, ``score()`` and FusedScorer -- against the fp64 model oracle.  Bounds: scores within 2e-5 of the score scale
(tests/test_gpu_packed_scorer.py, the fp64 oracle test of a mode-1 model); loss within 1e-5 (1 + |loss|) and every parameter
gradient within 2e-4 of the largest oracle gradient entry (tests/test_gpu_parity.py, test_fused_trainer_fc_sigmoid_tanh)."""
import copy

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from oracle import model_oracle as M
from tests.test_gpu_parity import _make_engine_model, _t

pytestmark = pytest.mark.gpu
F, B, L = 12, 3, 40
LENS = [40, 23, 7]


def _job(d, h):
    cfg = dict(n_features=F, fc_sizes=[d], fc_activation=None, fc_input_norm=False, N=1, d_ff=64, h=h, output_activation=None)
    params = M.init_params(cfg, seed=21)
    rng = np.random.default_rng(22)
    x = rng.standard_normal((B, L, F)).astype(np.float32)
    y = rng.integers(0, 5, (B, L)).astype(np.float32)
    for b, n in enumerate(LENS):
        x[b, n:], y[b, n:] = 0, -1
    return cfg, params, x, y


@pytest.mark.parametrize("d,h", [(128, 4), (48, 4)])
def test_narrow_heads_trainer_matches_the_fp64_oracle(d, h):
    from allrank_amd.engine import FusedTrainer
    cfg, params, x, y = _job(d, h)
    mask = y == -1
    model = _make_engine_model(cfg, params)
    ft = FusedTrainer(model, "listNet", {}, B, L, lr=1e-3, use_graph=False, narrow_heads=True)
    assert ft.attention_forward == "narrow" and ft.meta()["narrow_heads"] is True
    so, cache = M.forward(params, cfg, x, mask)
    lo, gs, _ = O.listnet(so, y)
    grads = M.backward(params, cfg, cache, gs)
    bar = 2e-5 * max(1.0, float(np.abs(so[~mask]).max()))
    sc = ft.score(_t(x), _t(y)).cpu().numpy()
    assert float(np.abs(sc - so)[~mask].max()) <= bar
    packed = ft.scorer(B, L).run(_t(x), _t(y), lengths=torch.tensor(LENS, dtype=torch.int32)).cpu().numpy()
    assert float(np.abs(packed - so)[~mask].max()) <= bar
    lf = float(ft.step(_t(x), _t(y)).item())
    assert abs(lf - float(lo)) <= 1e-5 * (1 + abs(float(lo))), (lf, lo)
    scale = max(float(np.abs(v).max()) for v in grads.values())
    for n, p_ in model.named_parameters():
        assert float(np.abs(p_.grad.cpu().numpy() - grads[n]).max()) <= 2e-4 * scale, n


def test_narrow_heads_off_is_the_default_engine_and_other_widths_ignore_it():
    from allrank_amd.engine import FusedTrainer
    cfg, params, x, y = _job(128, 4)
    model = _make_engine_model(cfg, params)
    off = FusedTrainer(copy.deepcopy(model), "listNet", {}, B, L, use_graph=False, narrow_heads=False)
    plain = FusedTrainer(copy.deepcopy(model), "listNet", {}, B, L, use_graph=False)
    assert off.attention_forward == plain.attention_forward == "default" and "narrow_heads" not in off.meta()
    assert off.meta() == plain.meta()
    assert torch.equal(off.score(_t(x), _t(y)), plain.score(_t(x), _t(y)))
    cfg, params, x, y = _job(128, 2)                              # head width 64: the resident kernels' range
    ft = FusedTrainer(_make_engine_model(cfg, params), "listNet", {}, B, L, use_graph=False, narrow_heads=True)
    assert ft.attention_forward == "default"
    assert torch.isfinite(ft.score(_t(x), _t(y))).all()
