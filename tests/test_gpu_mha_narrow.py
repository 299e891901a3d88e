"""The contract of the opt-in split-bf16 forward for head widths up to 32 (allrank_amd/csrc/ltrx_mha_narrow.hip), -m gpu.

ltrx_mha_fwd_narrow, then ltrx_mha_bwd of the same mode on its o / lse -- the exact kernels at these widths -- held to the entrywise
bars of tests/attention_ref.py for EVERY entry of O, lse, dQ, dK and dV, with the windows, sentinels and zero patterns of
tests/test_gpu_attention_contract.py (its `Problem`, with the forward call replaced).  Mode 2 must fail mode 1's bar on O.

  ltrx_mha_fwd_narrow_kernel<DROP=0/1, PL=0/1>    narrow dk4 / dk20 / dk32 ragged289 (modes 1 / 2)
  ltrx_mha_fwd_narrow_kernel<DROP=0/1, PL=0>      mask * narrow; climbing narrow

The ragged lengths give one key, a full 32-key group, one past it, one past a 128-key ring slot (and a second 128-query
workgroup), and the ring's wrap with a third workgroup.  The kernel keeps the lazy softmax reference of the resident forward
(kLazyTau = 8), so "climbing narrow" -- logits rising by 11 natural units per 32 keys -- is part of the table."""
import ctypes

import numpy as np
import pytest
import torch

from tests import attention_ref as A
from tests.test_gpu_attention_contract import CONSTS, EINVAL, EUNSUPPORTED, TAIL, WORD, Problem, _libs
from tests.test_gpu_gemm_contract import GARBAGE, Win
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

CASES = [A.Case("narrow dk%d ragged289" % dk, dk, 5, 289, 2, (0, .3), (1, 2), [1, 32, 33, 129, 289]) for dk in (4, 20, 32)]
CASES += [A.Case("mask %s narrow" % kind, 32, 2, 100, 2, (0, .3), (1,), None, kind, layouts=("padded",))
          for kind in ("first tile", "middle tile", "tail and interior", "slate")]
CASES += [A.Case("climbing narrow", 32, 2, 240, 2, (0, .3), (1,), [240, 230], family="climbing", layouts=("padded",))]


class NarrowProblem(Problem):
    def call(self, mode, p, seed=A.SEED):
        """`Problem.call` with ltrx_mha_fwd_narrow as the forward; the backward is ltrx_mha_bwd's exact arm"""
        LB, lib = _libs()
        c, d = self.c, self.d
        B, h, L, dk = c.B, c.h, c.L, c.dk
        what = "%s mode %d p %g" % (self.tag, mode, p)
        o = Win((self.R, d), self.ors, 4, np.nan)
        lse = Win((1, B * h * L), B * h * L, 8, np.nan)
        dqkv = Win((self.R, 3 * d), self.drs, 4, np.nan)
        nws = lib.ltrx_mha_bwd_workspace_bytes(B, L, h, dk, mode)
        assert nws == B * L * h * 4 == A.bwd_workspace_bytes(mode, B, L, h, dk, CONSTS), "%s: the backward is not the exact arm" % what
        ws = torch.full((nws + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
        q, k, v = self._p(self.qkv), self._p(self.qkv, d), self._p(self.qkv, 2 * d)
        st = LB.stream_of(ws)
        try:
            LB.check(lib.ltrx_mha_fwd_narrow(q, k, v, LB.ptr(self.mask), B, L, h, dk, self.rs, o.ptr, self.ors, lse.ptr, p, seed,
                                             LB.ptr(self.step), LB.ptr(self.cu), LB.ptr(self.order), mode, st), what + " fwd_narrow")
            LB.check(lib.ltrx_mha_bwd(q, k, v, LB.ptr(self.mask), o.ptr, self.do.ptr, lse.ptr, B, L, h, dk, self.rs, self.ors,
                                      self._p(dqkv), self._p(dqkv, d), self._p(dqkv, 2 * d), self.drs, p, seed, LB.ptr(self.step),
                                      LB.ptr(self.cu), LB.ptr(self.order), mode, LB.ptr(ws), st), what + " bwd")
            torch.cuda.synchronize()
        except RuntimeError as e:
            if "hip" in str(e).lower():
                pytest.exit("%s: %s -- nothing more is launched on a device that reported an error" % (what, e), returncode=3)
            raise
        assert bool((ws[nws:] == 0xA5).all()), "%s: the backward wrote behind its %d-byte workspace" % (what, nws)
        og, dg, lg = o.fetch(what + " o"), dqkv.fetch(what + " dq/dk/dv"), lse.fetch(what + " lse").reshape(B, h, L)

        def heads(rows2d):
            full = np.full((B * L, d), np.nan)
            full[self.sel] = rows2d
            return full.reshape(B, L, h, dk).transpose(0, 2, 1, 3)

        return dict(o=heads(og), lse=lg.astype(np.float64), dq=heads(dg[:, :d]), dk=heads(dg[:, d:2 * d]), dv=heads(dg[:, 2 * d:]))


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in CASES])
def test_narrow_forward_and_exact_backward_meet_the_entrywise_contract(c):
    """every (layout, mode, p) of the case: |kernel - fp64 reference| <= A.bars for every entry of the five tensors, NaN beyond a
    slate's length, exact zeros at padded keys and in a fully padded slate (`Problem.run`); mode 2 fails mode 1's bar on O; inputs
    unchanged."""
    X = A.Inputs(c)
    problems = [NarrowProblem(c, X, layout) for layout in c.layouts]
    for p in c.pdrops:
        ref = X.reference(p)
        bars = {mode: A.bars(ref, X.q, X.k, X.v, X.do, mode) for mode in sorted(set(c.modes) | {1})}
        for pr in problems:
            for mode in c.modes:
                pr.run(mode, p, ref, bars[mode], bars[1] if mode == 2 else None)
    for pr in problems:
        pr.inputs_unchanged()


def test_narrow_refusals_leave_the_outputs_untouched():
    LB, lib = _libs()
    B, L, h = 2, 40, 2
    mask = torch.zeros((B, L), dtype=torch.uint8, device=DEV)
    step = torch.full((1,), WORD, dtype=torch.int32, device=DEV)
    st = LB.stream_of(mask)
    for what, kw, want in [("mode 0", dict(mode=0), EINVAL), ("mode 3", dict(mode=3), EINVAL), ("d_k 36", dict(dk=36), EUNSUPPORTED),
                           ("d_k 30", dict(dk=30), EUNSUPPORTED), ("neither mask nor cu_seqlens", dict(mask=None), EINVAL)]:
        kw = dict(dict(dk=32, mode=1, mask=mask), **kw)
        d = h * kw["dk"]
        rs, ors = (3 * d + 11) // 4 * 4, (d + 7) // 4 * 4
        qkv = Win((B * L, 3 * d), rs, 4, GARBAGE, np.ones((B * L, 3 * d), np.float32))
        o = Win((B * L, d), ors, 4, np.nan)
        lse = Win((1, B * h * L), B * h * L, 8, np.nan)
        at = lambda col: ctypes.c_void_p(qkv.ptr.value + 4 * col)      # noqa: E731
        rc = lib.ltrx_mha_fwd_narrow(at(0), at(d), at(2 * d), LB.ptr(kw["mask"]), B, L, h, kw["dk"], rs, o.ptr, ors, lse.ptr, 0.3, A.SEED,
                                     LB.ptr(step), None, None, kw["mode"], st)
        assert rc == want, "%s: returned %d, expected %d" % (what, rc, want)
        torch.cuda.synchronize()
        for w in (qkv, o, lse):
            w.unchanged(what)
