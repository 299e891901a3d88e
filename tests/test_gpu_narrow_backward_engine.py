"""-m gpu: FusedTrainer(narrow_heads="both") -- the split-bf16 attention backward for head widths up to 32 (ltrx_mha_bwd_narrow) in the
training step -- against the fp64 model oracle with the bounds of tests/test_gpu_narrow_heads_engine.py (loss 1e-5, gradients 2e-4)."""
import copy

import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from oracle import model_oracle as M
from tests.test_gpu_parity import _make_engine_model, _t

pytestmark = pytest.mark.gpu
F, B, L = 12, 4, 40


@pytest.fixture(scope="module")
def job():
    cfg = dict(n_features=F, fc_sizes=[64], fc_activation=None, fc_input_norm=False, N=1, d_ff=64, h=2, output_activation=None)
    params = M.init_params(cfg, seed=21)
    rng = np.random.default_rng(22)
    x = rng.standard_normal((B, L, F)).astype(np.float32)
    y = rng.integers(0, 5, (B, L)).astype(np.float32)
    for b, n in enumerate([40, 23, 7, 1]):
        x[b, n:], y[b, n:] = 0, -1
    so, cache = M.forward(params, cfg, x, y == -1)
    lo, gs, _ = O.listnet(so, y)
    return _make_engine_model(cfg, params), _t(x), _t(y), float(lo), M.backward(params, cfg, cache, gs)


def _trainer(model, **kw):
    from allrank_amd.engine import FusedTrainer
    m = copy.deepcopy(model)                                    # (every trainer steps its own copy of the job's weights)
    return FusedTrainer(m, "listNet", {}, B, L, lr=1e-3, **kw), m


def test_both_and_true_match_the_fp64_oracle(job):
    """"both": the narrow backward, in the padded and the compact step; True: still the exact backward, on the same forward bits"""
    model, x, y, lo, grads = job
    scale = max(float(np.abs(v).max()) for v in grads.values())
    losses = []
    for narrow, backward, kw in (("both", "narrow", {}), (True, "default", {}), ("both", "narrow", dict(compact=True))):
        ft, m = _trainer(model, use_graph=False, narrow_heads=narrow, **kw)
        assert (ft.attention_forward, ft.attention_backward, ft.meta()["narrow_heads"]) == ("narrow", backward, narrow)
        losses.append(float(ft.step(x, y).item()))
        assert abs(losses[-1] - lo) <= 1e-5 * (1 + abs(lo)), (narrow, kw, losses[-1], lo)
        for n, p_ in m.named_parameters():
            assert float(np.abs(p_.grad.cpu().numpy() - grads[n]).max()) <= 2e-4 * scale, (narrow, kw, n)
    assert losses[0] == losses[1]
    with pytest.raises(ValueError, match="narrow_heads"):
        _trainer(model, narrow_heads="backward")


def test_the_captured_step_replays_the_eager_one_bit_for_bit(job):
    model, x, y, _, _ = job
    runs = []
    for use_graph in (False, True):
        ft, m = _trainer(model, use_graph=use_graph, narrow_heads="both")
        losses = [ft.step(x, y).clone() for _ in range(6)]      # (the third step captures; three replays follow)
        assert ft.attention_backward == "narrow" and (ft.graph is not None) == use_graph
        runs.append(losses + [p_.detach().clone() for p_ in m.parameters()] + [p_.grad.clone() for p_ in m.parameters()])
    assert all(torch.equal(u, v) for u, v in zip(*runs))
