"""The contract of the opt-in split-bf16 BACKWARD for head widths 65..128 (ltrx_mha_bwd_wide, allrank_amd/csrc/ltrx_mha_wide.hip), -m gpu.

ltrx_mha_fwd_wide, then ltrx_mha_bwd_wide on its o / lse, held to the entrywise bars of tests/attention_ref.py for EVERY entry of O, lse,
dQ, dK and dV through `Problem.run` of tests/test_gpu_attention_contract.py: NaN beyond a slate's length, exact zeros at padded keys
and in a fully padded slate, the 0xA5 sentinel behind the B L h 4-byte workspace, inputs unchanged.

  ltrx_mha_bwd_wide_{dq,dkdv}_kernel<96,  DROP=0/1, PL=0/1>    wide bwd dk68 / dk72 / dk96 ragged289 (modes 1 / 2)
  ltrx_mha_bwd_wide_{dq,dkdv}_kernel<128, DROP=0/1, PL=0/1>    wide bwd dk100 / dk124 / dk128 ragged289
  ltrx_mha_bwd_wide_{dq,dkdv}_kernel<96,  DROP=0/1, PL=0>      mask * wide bwd; exact forward, wide backward
Lengths 1 / 32 / 33 / 129 / 289: one key, a tile edge, a second 128-row block of one row (five tiles: both ring slots reused), ten tiles."""
import ctypes

import numpy as np
import pytest
import torch

from tests import attention_ref as A
from tests.test_gpu_attention_contract import EINVAL, EUNSUPPORTED, TAIL, WORD, Problem, _libs
from tests.test_gpu_gemm_contract import GARBAGE, Win
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

CASES = [A.Case("wide bwd dk%d ragged289" % dk, dk, 5, 289, 2, (0, .3), (1, 2), [1, 32, 33, 129, 289]) for dk in (68, 72, 96, 100, 124, 128)]
CASES += [A.Case("mask %s wide bwd" % kind, 96, 2, 100, 2, (0, .3), (1,), None, kind, layouts=("padded",))
          for kind in ("first tile", "middle tile", "tail and interior", "slate")]
EXACT_FWD = A.Case("exact forward, wide backward", 96, 3, 130, 2, (0, .3), (1,), [1, 33, 130])


class WideBwdProblem(Problem):
    def call(self, mode, p, seed=A.SEED):
        """`Problem.call` with `self.forward` as the forward and ltrx_mha_bwd_wide as the backward"""
        LB, lib = _libs()
        c, d = self.c, self.d
        B, h, L, dk = c.B, c.h, c.L, c.dk
        what = "%s mode %d p %g" % (self.tag, mode, p)
        o = Win((self.R, d), self.ors, 4, np.nan)
        lse = Win((1, B * h * L), B * h * L, 8, np.nan)
        dqkv = Win((self.R, 3 * d), self.drs, 4, np.nan)
        nws = lib.ltrx_mha_bwd_workspace_bytes(B, L, h, dk, mode)
        assert nws == B * L * h * 4, what
        ws = torch.full((nws + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
        q, k, v = self._p(self.qkv), self._p(self.qkv, d), self._p(self.qkv, 2 * d)
        st = LB.stream_of(ws)
        try:
            LB.check(getattr(lib, self.forward)(q, k, v, LB.ptr(self.mask), B, L, h, dk, self.rs, o.ptr, self.ors, lse.ptr, p, seed,
                                                LB.ptr(self.step), LB.ptr(self.cu), LB.ptr(self.order), mode, st), what + " " + self.forward)
            LB.check(lib.ltrx_mha_bwd_wide(q, k, v, LB.ptr(self.mask), o.ptr, self.do.ptr, lse.ptr, B, L, h, dk, self.rs, self.ors,
                                           self._p(dqkv), self._p(dqkv, d), self._p(dqkv, 2 * d), self.drs, p, seed, LB.ptr(self.step),
                                           LB.ptr(self.cu), LB.ptr(self.order), mode, LB.ptr(ws), st), what + " bwd_wide")
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


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in CASES + [EXACT_FWD]])
def test_wide_backward_meets_the_entrywise_contract(c):
    X = A.Inputs(c)
    problems = [WideBwdProblem(c, X, layout) for layout in c.layouts]
    for pr in problems:
        pr.forward = "ltrx_mha_fwd" if c is EXACT_FWD else "ltrx_mha_fwd_wide"      # (the exact arm at these widths: interchangeable)
    for p in c.pdrops:
        ref = X.reference(p)
        bars = {mode: A.bars(ref, X.q, X.k, X.v, X.do, mode) for mode in sorted(set(c.modes) | {1})}
        for pr in problems:
            for mode in c.modes:
                pr.run(mode, p, ref, bars[mode], bars[1] if mode == 2 else None)
    for pr in problems:
        pr.inputs_unchanged()


def test_wide_backward_refusals_leave_the_outputs_untouched():
    LB, lib = _libs()
    B, L, h = 2, 40, 2
    mask = torch.zeros((B, L), dtype=torch.uint8, device=DEV)
    step = torch.full((1,), WORD, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    st = LB.stream_of(ws)
    for what, kw, want in [("mode 0", dict(mode=0), EINVAL), ("mode 3", dict(mode=3), EINVAL), ("d_k 64", dict(dk=64), EUNSUPPORTED),
                           ("d_k 132", dict(dk=132), EUNSUPPORTED), ("d_k 70", dict(dk=70), EUNSUPPORTED), ("NULL lse", dict(lse=False), EINVAL)]:
        kw = dict(dict(dk=96, mode=1, lse=True), **kw)
        d = h * kw["dk"]
        rs, ors = (3 * d + 11) // 4 * 4, (d + 7) // 4 * 4
        qkv = Win((B * L, 3 * d), rs, 4, GARBAGE, np.ones((B * L, 3 * d), np.float32))
        o = Win((B * L, d), ors, 4, GARBAGE, np.ones((B * L, d), np.float32))
        lse = Win((1, B * h * L), B * h * L, 8, GARBAGE, np.ones((1, B * h * L), np.float32))
        dqkv = Win((B * L, 3 * d), rs, 4, np.nan)
        at = lambda w, col=0: ctypes.c_void_p(w.ptr.value + 4 * col)      # noqa: E731
        rc = lib.ltrx_mha_bwd_wide(at(qkv), at(qkv, d), at(qkv, 2 * d), LB.ptr(mask), o.ptr, o.ptr, lse.ptr if kw["lse"] else None, B, L, h,
                                   kw["dk"], rs, ors, at(dqkv), at(dqkv, d), at(dqkv, 2 * d), rs, 0.3, A.SEED, LB.ptr(step), None, None,
                                   kw["mode"], LB.ptr(ws), st)
        assert rc == want, "%s: returned %d, expected %d" % (what, rc, want)
        torch.cuda.synchronize()
        for w in (qkv, o, lse, dqkv):
            w.unchanged(what)
    assert not bool(ws.any()), "a refused backward wrote its workspace"
