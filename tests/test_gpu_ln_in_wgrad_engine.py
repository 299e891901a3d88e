"""-m gpu: FusedTrainer(ln_in_wgrad=True) -- the first-sublayer LayerNorm backward of every encoder layer inside the layer's grouped
weight-gradient launch (ltrx_gemm_tn_group_ln), the residual-stream gradient rotating over three buffers -- against ln_in_wgrad=False
(the two launches, two buffers): loss, scores and every parameter BIT-EQUAL after one and after three steps, captured and eager.

Shape: two layers, d_model 256, d_ff 256, 8 slates x 256 items = 2048 rows, the smallest row count at which the four projections run
as ONE grouped launch (6 tiles x 16 splits = 96 workgroups, ltrx_debug_tn_group_map): the side job is taken.  The dropout case runs
32 x 256 = 8192 rows: with both residual dropouts on, a layer's weight gradients run as two launches and the second one (attention
output + qkv: 4 tiles x 64 splits) fills all 256 CUs, so the call falls back to its two-launch form -- the engine does not see it."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, F, D = 256, 24, 256


def _model(dropout):
    from allrank_amd.model import make_model
    torch.manual_seed(11)
    return make_model(dict(sizes=[D], input_norm=False, activation=None, dropout=0.0),
                      dict(N=2, d_ff=256, h=4, positional_encoding=None, dropout=dropout), dict(d_output=1, output_activation=None), F).to(DEV)


def _batches(B, n):
    rng = np.random.default_rng(21)
    out = []
    for _ in range(n):
        x = rng.standard_normal((B, L, F)).astype(np.float32)
        y = rng.integers(0, 5, (B, L)).astype(np.float32)
        out.append((torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)))
    return out


def _layer_wgs(B, probs):
    from allrank_amd import _lib
    n = len(probs)
    NP = (ctypes.c_int * n)(*[a for a, _ in probs])
    KP = (ctypes.c_int * n)(*[b for _, b in probs])
    t_out, s_out = (ctypes.c_ubyte * 256)(), (ctypes.c_ubyte * 256)()
    return _lib.lib().ltrx_debug_tn_group_map(n, B * L, NP, KP, t_out, s_out)


def _run(B, dropout, use_graph, steps):
    from allrank_amd.engine import FusedTrainer
    m_on = _model(dropout)
    m_off = copy.deepcopy(m_on)
    kw = dict(lr=1e-3, use_graph=use_graph, seed=3)
    on = FusedTrainer(m_on, "approxNDCGLoss", {}, B, L, **kw)
    off = FusedTrainer(m_off, "approxNDCGLoss", {}, B, L, ln_in_wgrad=False, **kw)
    assert on.ln_in_wgrad and hasattr(on, "d_c") and not off.ln_in_wgrad and not hasattr(off, "d_c")
    for i, (x, y) in enumerate(_batches(B, steps)):
        l_on, l_off = on.step(x, y, None).clone(), off.step(x, y, None).clone()
        assert torch.equal(l_on, l_off) and bool(torch.isfinite(l_on).all()), (i, l_on, l_off)
        assert torch.equal(on.scores, off.scores), i
    p_off = dict(m_off.named_parameters())
    g_on, g_off = {id(r.p): r.g for r in on.params}, {id(r.p): r.g for r in off.params}
    for n_, p in m_on.named_parameters():
        assert torch.equal(p.data, p_off[n_].data), n_
        assert torch.equal(g_on[id(p)], g_off[id(p_off[n_])]), n_
    assert all(took for _, took in on.wgrad_group_log), on.wgrad_group_log
    return on, off


@pytest.mark.parametrize("use_graph", [True, False], ids=["captured", "eager"])
@pytest.mark.parametrize("steps", [1, 3])
def test_steps_with_the_side_job_equal_the_steps_without_it(use_graph, steps):
    assert _layer_wgs(8, [(256, 256), (256, 256), (256, 256), (768, 256)]) == 96       # the grouped launch, 160 CUs free
    assert _layer_wgs(8, [(256, 256), (256, 256), (256, 256), (768, 256)][:3]) > 0
    on, off = _run(8, 0.0, use_graph, steps)
    assert on.ln_side_log and all(s == 160 for s in on.ln_side_log), on.ln_side_log  # both layers took it
    assert off.ln_side_log == []


def test_dropout_fills_the_launch_and_the_call_falls_back():
    assert _layer_wgs(32, [(256, 256), (768, 256)]) == 256                            # attention output + qkv: no CU left
    on, off = _run(32, 0.1, True, 3)
    assert on.ln_side_log and all(s == 0 for s in on.ln_side_log), on.ln_side_log
