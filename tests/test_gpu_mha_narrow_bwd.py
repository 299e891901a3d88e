"""The contract of the opt-in split-bf16 BACKWARD for head widths up to 32 (ltrx_mha_bwd_narrow, allrank_amd/csrc/ltrx_mha_narrow.hip), -m gpu.

ltrx_mha_fwd_narrow, then ltrx_mha_bwd_narrow on its o / lse, held to the entrywise bars of tests/attention_ref.py for EVERY entry of O,
lse, dQ, dK and dV through `Problem.run` of tests/test_gpu_attention_contract.py (NaN beyond a slate's length, exact zeros at padded
keys and in a fully padded slate, the 0xA5 sentinel behind the workspace, inputs unchanged; mode 2 must fail mode 1's bar on O).
Lengths 1 / 32 / 33 / 129 / 289: one key, a full group, one past it, one past a ring slot, the ring's wrap; the masks at L 289 leave
whole key groups off (skipped) and whole 32-key blocks of a wave off (zero rows)."""
import numpy as np
import pytest
import torch

from tests import attention_ref as A
from tests.test_gpu_attention_contract import EINVAL, EUNSUPPORTED, TAIL, WORD, Problem, _libs
from tests.test_gpu_gemm_contract import GARBAGE, Win
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

CASES = [A.Case("narrow bwd dk%d ragged289" % dk, dk, 5, 289, 2, (0, .3), (1, 2), [1, 32, 33, 129, 289]) for dk in (4, 12, 16, 28, 32)]
CASES += [A.Case("mask %s narrow bwd" % kind, 32, 2, 289, 2, (0, .3), (1,), None, kind, layouts=("padded",))
          for kind in ("first tile", "middle tile", "tail and interior", "slate")]
CASES += [A.Case("climbing narrow bwd", 32, 2, 240, 2, (0, .3), (1,), [240, 230], family="climbing", layouts=("padded",))]
EXACT_FWD = A.Case("exact forward, narrow backward", 32, 3, 130, 2, (0, .3), (1,), [1, 33, 130])


class NarrowBwdProblem(Problem):
    def call(self, mode, p, seed=A.SEED):
        """`Problem.call` with `self.forward` as the forward and ltrx_mha_bwd_narrow as the backward"""
        LB, lib = _libs()
        (B, h, L, dk), d = (self.c.B, self.c.h, self.c.L, self.c.dk), self.d
        what = "%s mode %d p %g" % (self.tag, mode, p)
        o, lse, dqkv = Win((self.R, d), self.ors, 4, np.nan), Win((1, B * h * L), B * h * L, 8, np.nan), Win((self.R, 3 * d), self.drs, 4, np.nan)
        nws = lib.ltrx_mha_bwd_workspace_bytes(B, L, h, dk, mode)
        assert nws == B * L * h * 4, what
        ws = torch.full((nws + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
        qkv, dx = [self._p(self.qkv, j * d) for j in range(3)], [self._p(dqkv, j * d) for j in range(3)]
        rest = (p, seed, LB.ptr(self.step), LB.ptr(self.cu), LB.ptr(self.order), mode)
        st = LB.stream_of(ws)
        try:
            LB.check(getattr(lib, self.forward)(*qkv, LB.ptr(self.mask), B, L, h, dk, self.rs, o.ptr, self.ors, lse.ptr, *rest, st),
                     what + " " + self.forward)
            LB.check(lib.ltrx_mha_bwd_narrow(*qkv, LB.ptr(self.mask), o.ptr, self.do.ptr, lse.ptr, B, L, h, dk, self.rs, self.ors, *dx, self.drs,
                                             *rest, LB.ptr(ws), st), what + " bwd_narrow")
            torch.cuda.synchronize()
        except RuntimeError as e:
            if "hip" in str(e).lower():
                pytest.exit("%s: %s -- nothing more is launched on a device that reported an error" % (what, e), returncode=3)
            raise
        assert bool((ws[nws:] == 0xA5).all()), "%s: the backward wrote behind its %d-byte workspace" % (what, nws)
        og, dg, lg = o.fetch(what + " o"), dqkv.fetch(what + " dq/dk/dv"), lse.fetch(what + " lse").reshape(B, h, L)
        full = np.full((4, B * L, d), np.nan)                      # o, dq, dk, dv as [B, h, L, d_k], NaN at rows the layout does not hold
        full[:, self.sel] = np.stack([og, dg[:, :d], dg[:, d:2 * d], dg[:, 2 * d:]])
        return dict(zip(("o", "dq", "dk", "dv"), full.reshape(4, B, L, h, dk).transpose(0, 1, 3, 2, 4)), lse=lg.astype(np.float64))


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in CASES + [EXACT_FWD]])
def test_narrow_backward_meets_the_entrywise_contract(c):
    X = A.Inputs(c)
    problems = [NarrowBwdProblem(c, X, layout) for layout in c.layouts]
    for pr in problems:
        pr.forward = "ltrx_mha_fwd" if c is EXACT_FWD else "ltrx_mha_fwd_narrow"      # (the exact arm at these widths: interchangeable)
    for p in c.pdrops:
        ref = X.reference(p)
        bars = {mode: A.bars(ref, X.q, X.k, X.v, X.do, mode) for mode in sorted(set(c.modes) | {1})}
        for pr in problems:
            for mode in c.modes:
                pr.run(mode, p, ref, bars[mode], bars[1] if mode == 2 else None)
    for pr in problems:
        pr.inputs_unchanged()


def test_narrow_backward_refusals_leave_the_outputs_untouched():
    LB, lib = _libs()
    B, L, h = 2, 40, 2
    mask, step = torch.zeros((B, L), dtype=torch.uint8, device=DEV), torch.full((1,), WORD, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    for what, kw, want in [("mode 0", dict(mode=0), EINVAL), ("d_k 36", dict(dk=36), EUNSUPPORTED), ("d_k 6", dict(dk=6), EUNSUPPORTED),
                           ("NULL ws", dict(ws=None), EINVAL)]:
        kw = dict(dict(dk=32, mode=1, ws=ws), **kw)
        d = h * kw["dk"]
        rs, ors = (3 * d + 11) // 4 * 4, (d + 7) // 4 * 4
        qkv, dqkv = Win((B * L, 3 * d), rs, 4, GARBAGE, np.ones((B * L, 3 * d), np.float32)), Win((B * L, 3 * d), rs, 4, np.nan)
        o = Win((B * L, d), ors, 4, GARBAGE, np.ones((B * L, d), np.float32))
        lse = Win((1, B * h * L), B * h * L, 8, GARBAGE, np.ones((1, B * h * L), np.float32))
        at = lambda w: [w.ptr.value + 4 * d * j for j in range(3)]      # noqa: E731
        rc = lib.ltrx_mha_bwd_narrow(*at(qkv), LB.ptr(mask), o.ptr, o.ptr, lse.ptr, B, L, h, kw["dk"], rs, ors, *at(dqkv), rs, 0.3, A.SEED,
                                     LB.ptr(step), None, None, kw["mode"], LB.ptr(kw["ws"]), LB.stream_of(ws))
        assert rc == want, "%s: returned %d, expected %d" % (what, rc, want)
        torch.cuda.synchronize()
        for w in (qkv, o, lse, dqkv):
            w.unchanged(what)
    assert not bool(ws.any()), "a refused backward wrote its workspace"
