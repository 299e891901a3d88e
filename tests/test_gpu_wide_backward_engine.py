"""-m gpu: FusedTrainer(wide_backward=True) -- the split-bf16 attention backward for head widths 65..128 (ltrx_mha_bwd_wide) in the
training step -- against the fp64 model oracle, on the job and with the bounds of tests/test_gpu_wide_heads_engine.py: loss within
1e-5 (1 + |loss|), every parameter gradient within 2e-4 of the largest oracle gradient entry."""
import copy

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from oracle import model_oracle as M
from tests.test_gpu_parity import _make_engine_model, _t
from tests.test_gpu_wide_heads_engine import B, L, _job

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d,h", [(96, 1), (144, 2)])
def test_wide_backward_trainer_matches_the_fp64_oracle(d, h):
    from allrank_amd.engine import FusedTrainer
    cfg, params, x, y = _job(d, h)
    mask = y == -1
    model = _make_engine_model(cfg, params)
    ft = FusedTrainer(model, "listNet", {}, B, L, lr=1e-3, use_graph=False, wide_heads=True, wide_backward=True)
    assert ft.attention_backward == "wide" and ft.meta()["wide_backward"] is True
    so, cache = M.forward(params, cfg, x, mask)
    lo, gs, _ = O.listnet(so, y)
    grads = M.backward(params, cfg, cache, gs)
    lf = float(ft.step(_t(x), _t(y)).item())
    assert abs(lf - float(lo)) <= 1e-5 * (1 + abs(float(lo))), (lf, lo)
    scale = max(float(np.abs(v).max()) for v in grads.values())
    for n, p_ in model.named_parameters():
        assert float(np.abs(p_.grad.cpu().numpy() - grads[n]).max()) <= 2e-4 * scale, n


def test_wide_backward_off_is_the_default_engine_and_other_widths_ignore_it():
    from allrank_amd.engine import FusedTrainer
    cfg, params, x, y = _job(96, 1)
    model = _make_engine_model(cfg, params)
    got = []
    for kw in (dict(wide_backward=False), dict()):
        m = copy.deepcopy(model)
        ft = FusedTrainer(m, "listNet", {}, B, L, use_graph=False, **kw)
        assert ft.attention_backward == "default" and "wide_backward" not in ft.meta()
        ft.step(_t(x), _t(y))
        got.append([p_.grad.clone() for p_ in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*got))
    cfg, params, x, y = _job(128, 2)                              # head width 64: the resident kernels' range
    ft = FusedTrainer(_make_engine_model(cfg, params), "listNet", {}, B, L, use_graph=False, wide_backward=True)
    assert ft.attention_backward == "default"
