"""The attention contract's own evidence, without a GPU (tests/attention_ref.py): honest fp32 attention stays far below the bars,
every defect model is above them on every case it applies to, the reference is the oracle's, and the case table reaches every
dispatch arm and every kernel instantiation of ltrx_mha.hip / ltrx_mha_res.hip."""
import math

import numpy as np
import pytest
import torch

from oracle import model_oracle as M
from tests import attention_ref as A

CPU_CASES = [A.cpu_core(c) for c in A.CASES]
_CACHE = {}


def _setup(c, p):
    """inputs, reference and mode-0 bars of (case, p_drop): built once, shared by the tests below, never modified"""
    key = (c.name, p)
    if key not in _CACHE:
        if len(_CACHE) > 3:
            _CACHE.clear()
        X = A.Inputs(c)
        ref = X.reference(p)
        _CACHE[key] = (X, ref, A.bars(ref, X.q, X.k, X.v, X.do, 0))
    return _CACHE[key]


def _torch_fp32(X, p):
    """plain fp32 attention with autograd; a fully padded slate gives 0 as the kernels document"""
    q, k, v = (torch.tensor(x, requires_grad=True) for x in (X.q, X.k, X.v))
    mask = torch.tensor(X.mask)
    full = mask.all(-1)
    mk = mask & ~full[:, None]
    s = (q @ k.transpose(-1, -2)) / math.sqrt(X.c.dk)
    s = s.masked_fill(mk[:, None, None, :], float("-inf"))
    pr = torch.softmax(s, -1)
    keep = X.keep(p)
    o = (pr * torch.tensor(keep) if keep is not None else pr) @ v
    lse = torch.logsumexp(s, -1)
    live = (~full)[:, None, None, None].to(o.dtype)
    (o * torch.tensor(X.do) * live).sum().backward()
    out = dict(o=(o * live).detach(), lse=(lse * live[..., 0]).detach(), dq=q.grad, dk=k.grad, dv=v.grad)
    out = {t: a.numpy().astype(np.float64) for t, a in out.items()}
    for t in ("dq", "dk", "dv"):
        out[t][full.numpy()] = 0.0
    return out


def _ids():
    return [pytest.param(c, p, id="%s p%g" % (c.name, p)) for c in CPU_CASES for p in c.pdrops]


@pytest.mark.parametrize("c,p", _ids())
def test_fp32_attention_is_far_below_the_bar_and_every_defect_model_is_above_it(c, p):
    X, ref, bar = _setup(c, p)
    got = _torch_fp32(X, p)
    for t in A.TENSORS:
        ratio, idx, err, b = A.worst(got[t], getattr(ref, t), bar[t])
        assert ratio <= 0.25, "%s p %g: fp32 %s at %s is off by %.3g against a bar of %.3g (ratio %.3g)" % (c.name, p, t, idx, err, b, ratio)
    cp = c._replace(p=p)
    for name, (model, applies) in A.DEFECTS.items():
        if not applies(cp, X):
            continue
        bad = model(cp, X)
        ratios = {t: A.worst(bad[t], getattr(ref, t), bar[t])[0] for t in A.TENSORS}
        assert max(ratios.values()) > 1.0, "%s p %g: the defect '%s' stays inside every bar: %r" % (c.name, p, name, ratios)
        if 1 in c.modes:                                 # cases held to the mode-1 bar must tell the defects apart there, too
            bar1 = A.bars(ref, X.q, X.k, X.v, X.do, 1)
            assert max(A.worst(bad[t], getattr(ref, t), bar1[t])[0] for t in A.TENSORS) > 1.0, (c.name, p, name)


def test_every_defect_model_applies_somewhere():
    hit = set()
    for c in CPU_CASES:
        if c.B > 100:
            continue
        X = A.Inputs(c)
        for p in c.pdrops:
            hit |= {name for name, (_, applies) in A.DEFECTS.items() if applies(c._replace(p=p), X)}
    assert hit == set(A.DEFECTS)


def test_reference_is_the_oracle_and_its_fully_padded_convention_is_pinned():
    c = [c for c in CPU_CASES if c.name == "mask slate resident"][0]
    X = A.Inputs(c)
    keep = X.keep(0.3)
    ref = X.reference(0.3)
    q, k, v, do = (x.astype(np.float64) for x in (X.q, X.k, X.v, X.do))
    o, p = M.attention_fwd(q[:1], k[:1], v[:1], X.mask[:1], keep[:1].astype(np.float64))
    dq, dk, dv = M.attention_bwd(q[:1], k[:1], v[:1], p, do[:1], keep[:1].astype(np.float64))
    for got, want in ((ref.o, o), (ref.dq, dq), (ref.dk, dk), (ref.dv, dv)):
        assert np.abs(got[:1] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    s = np.where(X.mask[0][None, None, :], -np.inf, q[0] @ np.swapaxes(k[0], -1, -2) / math.sqrt(c.dk))
    lse = np.log(np.exp(s - s.max(-1, keepdims=True)).sum(-1)) + s.max(-1)
    assert np.abs(ref.lse[0] - lse).max() <= 1e-12 * np.abs(lse).max()
    # slate 1 is fully padded: zeros everywhere, lse 0, and bars of 0 (the kernels must write exact zeros)
    bar = A.bars(ref, X.q, X.k, X.v, X.do, 1)
    for t in A.TENSORS:
        assert (getattr(ref, t)[1] == 0).all() and (bar[t][1] == 0).all(), t
        assert np.isfinite(getattr(ref, t)).all() and np.isfinite(bar[t]).all(), t
    # the [L, d_k] form of one (slate, head)
    one = A.reference(X.q[0, 1], X.k[0, 1], X.v[0, 1], X.do[0, 1], X.mask[0], keep[0, 1])
    for t in A.TENSORS:
        assert np.array_equal(getattr(one, t), getattr(ref, t)[0, 1]), t
    # the hook-free variant (the defect models' base) is the same function
    base = A.variant(X.q, X.k, X.v, X.do, X.mask, keep)
    for t in A.TENSORS:
        want = getattr(ref, t)
        assert np.abs(base[t] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), t


def test_padded_key_rows_have_a_bar_of_zero():
    c = [c for c in CPU_CASES if c.name == "mask tail and interior exact"][0]
    X = A.Inputs(c)
    ref = X.reference(0.3)
    bar = A.bars(ref, X.q, X.k, X.v, X.do, 0)
    rows = np.broadcast_to(X.mask[:, None, :, None], ref.dk.shape)
    assert rows.any() and (bar["dk"][rows] == 0).all() and (bar["dv"][rows] == 0).all()
    assert (ref.dk[rows] == 0).all() and (ref.dv[rows] == 0).all()


def test_case_table_reaches_every_arm_and_every_instantiation():
    consts = A.header_constants()
    assert consts == dict(LTRX_MAX_SLATE_LEN=2048, LTRX_MHA_DS_BUDGET_BYTES=2 ** 31)
    arms, inst, nw = set(), set(), set()
    for c in A.CASES:
        for mode in c.modes:
            arm = A.arm_name(mode, c.B, c.L, c.h, c.dk, consts)
            arms.add((arm, mode))
            for p in c.pdrops:
                inst |= A.instantiations(mode, c.B, c.L, c.h, c.dk, p, consts)
    assert arms == {("exact", 0), ("exact", 1), ("res", 1), ("res", 2), ("mixed", 1), ("mixed", 2)}
    missing = A.all_instantiations() - inst
    assert not missing and len(A.all_instantiations()) == 36, sorted(missing)
    # the two reasons for the mixed arm, and the workspace each arm asks for
    big = [c for c in A.CASES if c.name == "mixed budget"][0]
    assert A.bwd_arm(1, big.B, big.L, big.h, big.dk, consts) == "exact" and A.bwd_arm(1, big.B - 1, big.L, big.h, big.dk, consts) == "res"
    assert A.bwd_workspace_bytes(1, big.B, big.L, big.h, big.dk, consts) == big.B * big.L * big.h * 4
    assert A.bwd_workspace_bytes(1, big.B - 1, big.L, big.h, big.dk, consts) == (big.B - 1) * 64 * 64 * 4
    assert A.bwd_arm(1, 1, 2048, 1, 36, consts) == "res" and A.bwd_arm(1, 1, 2049, 1, 36, consts) == "exact"
    assert A.bwd_arm(1, 2, 161, 2, 64, consts) == "res" and A.bwd_arm(0, 2, 161, 2, 64, consts) == "exact"
    assert A.fwd_arm(1, 32) == "exact" and A.fwd_arm(1, 36) == "res" and A.fwd_arm(2, 64) == "res" and A.fwd_arm(1, 68) == "exact"


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415927, 3.0e37], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.140625, float(torch.tensor(3.0e37).bfloat16().float())])
    assert np.array_equal(A.bf16(x), want)
    r = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(A.bf16(r), torch.tensor(r).bfloat16().float().numpy().astype(np.float64))
