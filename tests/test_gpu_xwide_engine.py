"""-m gpu: the fused engine on a model of head width 256 (fc [256] + one encoder layer d 256, h 1, d_ff 64; ltrx_mha_fwd_xwide /
ltrx_mha_bwd_xwide) against the fp64 model oracle, in the padded, the compact and the captured step (the capturing visit and a replay,
at learning rate 0 so that each starts from the oracle's weights), with the bounds of
tests/test_gpu_wide_heads_engine.py: loss within 1e-5 (1 + |loss|), every parameter gradient within 2e-4 of the largest oracle
gradient entry.  Before these kernels FusedTrainer refused the model and rank_slates took the nn.Module path."""
import numpy as np
import pytest
import torch

from oracle import ltr_oracle as O
from oracle import model_oracle as M
from tests import rank_cases as RC
from tests.test_gpu_parity import _make_engine_model, _t

pytestmark = pytest.mark.gpu
F, B, L, D = 12, 4, 40, 256
LENS = [40, 23, 7, 31]


def _job():
    cfg = dict(n_features=F, fc_sizes=[D], fc_activation=None, fc_input_norm=False, N=1, d_ff=64, h=1, output_activation=None)
    params = M.init_params(cfg, seed=21)
    rng = np.random.default_rng(22)
    x = rng.standard_normal((B, L, F)).astype(np.float32)
    y = rng.integers(0, 5, (B, L)).astype(np.float32)
    for b, n in enumerate(LENS):
        x[b, n:], y[b, n:] = 0, -1
    return cfg, params, x, y


@pytest.fixture(scope="module")
def oracle():
    cfg, params, x, y = _job()
    so, cache = M.forward(params, cfg, x, y == -1)
    lo, gs, _ = O.listnet(so, y)
    return cfg, params, x, y, float(lo), M.backward(params, cfg, cache, gs)


@pytest.mark.parametrize("kw", [dict(use_graph=False), dict(compact=True, use_graph=False), dict(use_graph=True)], ids=["padded", "compact", "captured"])
def test_xwide_step_matches_the_fp64_oracle(oracle, kw):
    from allrank_amd.engine import FusedTrainer
    cfg, params, x, y, lo, grads = oracle
    model = _make_engine_model(cfg, params)
    ft = FusedTrainer(model, "listNet", {}, B, L, lr=0.0, **kw)      # (lr 0: every step starts from the oracle's weights)
    assert ft.attention_forward == ft.attention_backward == "xwide"
    start = [p_.detach().clone() for p_ in model.parameters()]
    scale = max(float(np.abs(v).max()) for v in grads.values())
    modes = []
    for _ in range(4 if kw["use_graph"] else 1):          # a graph's first two visits are eager warm-ups: then the capture, then a replay
        lf = float(ft.step(_t(x), _t(y)).item())
        assert all(torch.equal(p_, s) for p_, s in zip(model.parameters(), start))
        modes.append(ft.last_mode)
        assert abs(lf - lo) <= 1e-5 * (1 + abs(lo)), (modes, lf, lo)
        for n, p_ in model.named_parameters():
            assert float(np.abs(p_.grad.cpu().numpy() - grads[n]).max()) <= 2e-4 * scale, (modes, n)
    assert modes == (["eager", "eager", "capture", "replay"] if kw["use_graph"] else ["eager"])


def test_rank_slates_scores_the_model_on_the_fused_engine(oracle):
    from allrank_amd import inference as EI
    cfg, params, x, y = oracle[:4]
    EI.rank_slates({"vali": RC.HostSlates(x, y)}, _make_engine_model(cfg, params), RC.config(B))
    assert EI.last_run["engine"] == "fused" and EI.last_run["reason"] == "", EI.last_run
