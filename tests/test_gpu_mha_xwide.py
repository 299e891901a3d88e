"""The contract of the split-bf16 attention for head widths 132..256 (ltrx_mha_fwd_xwide / ltrx_mha_bwd_xwide, ltrx_mha_xwide.hip), -m gpu.

ltrx_mha_fwd_xwide, then ltrx_mha_bwd_xwide on its o / lse, held to the entrywise bars of tests/attention_ref.py for EVERY entry of O,
lse, dQ, dK and dV through `Problem.run` of tests/test_gpu_attention_contract.py (NaN beyond a slate's length, exact zeros at padded
keys and in a fully padded slate, the 0xA5 sentinel behind the B L h floats of workspace, inputs unchanged; mode 2 is held to the
one-product bar and must fail mode 1's on O).  d_k 132 / 160 / 256: the smallest width, one that is no multiple of 32 columns short
of its padding, the maximum.  Lengths 1 / 33 / 129 / 300 (1 and 33 also as the L of a padded batch): below one key tile, across a tile edge, more than one 64-row block, five
turns of the two-slot ring; length 0 is the fully padded slate of the padded layout and the empty one of cu_seqlens, which is
visited in a shuffled slate_order.  Forward and backward draw the dropout mask from the same (seed, step word)."""
import numpy as np
import pytest
import torch

from tests import attention_ref as A
from tests.test_gpu_attention_contract import EINVAL, EUNSUPPORTED, TAIL, WORD, Problem, _libs
from tests.test_gpu_gemm_contract import GARBAGE, Win
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

CASES = [A.Case("xwide dk%d h%d L%d" % (dk, h, L), dk, 3, L, h, (0, .3), (1, 2), lens)._replace(strides="own")
         for dk in (132, 160, 256) for h in (1, 2) for L, lens in ((300, [300, 129, 0]), (40, [33, 0, 1]))]
# the padded layout at L = 1 and 33 itself (the kernels' `len` is L there: below one key tile, one key past it), with a key mask
CASES += [A.Case("xwide dk%d h%d padded L%d" % (dk, h, L), dk, 3, L, h, (0, .3), modes, lens, layouts=("padded",))._replace(strides="own")
          for dk, h in ((132, 2), (160, 1), (256, 1)) for L, lens, modes in ((1, [1, 0, 1], (1,)), (33, [33, 20, 0], (1, 2)))]


class XwideProblem(Problem):
    def launch(self, mode, p, o, lse, dqkv, ws, seed=A.SEED):
        LB, lib = _libs()
        (B, h, L, dk), d = (self.c.B, self.c.h, self.c.L, self.c.dk), self.d
        qkv, dx = [self._p(self.qkv, j * d) for j in range(3)], [self._p(dqkv, j * d) for j in range(3)]
        rest = (p, seed, LB.ptr(self.step), LB.ptr(self.cu), LB.ptr(self.order), mode)
        st = LB.stream_of(ws)
        LB.check(lib.ltrx_mha_fwd_xwide(*qkv, LB.ptr(self.mask), B, L, h, dk, self.rs, o.ptr, self.ors, lse.ptr, *rest, st), "fwd_xwide")
        LB.check(lib.ltrx_mha_bwd_xwide(*qkv, LB.ptr(self.mask), o.ptr, self.do.ptr, lse.ptr, B, L, h, dk, self.rs, self.ors, *dx, self.drs,
                                        *rest, LB.ptr(ws), st), "bwd_xwide")

    def call(self, mode, p, seed=A.SEED):
        """`Problem.call` on the two xwide entries; the backward runs twice into windows of its own and must give the same bits"""
        _, lib = _libs()
        (B, h, L, dk), d = (self.c.B, self.c.h, self.c.L, self.c.dk), self.d
        what = "%s mode %d p %g" % (self.tag, mode, p)
        o, lse = Win((self.R, d), self.ors, 4, np.nan), Win((1, B * h * L), B * h * L, 8, np.nan)
        dqkv, again = Win((self.R, 3 * d), self.drs, 4, np.nan), Win((self.R, 3 * d), self.drs, 4, np.nan)
        nws = lib.ltrx_mha_bwd_workspace_bytes(B, L, h, dk, mode)
        assert nws == B * L * h * 4, what
        ws = torch.full((nws + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
        try:
            self.launch(mode, p, o, lse, dqkv, ws, seed)
            self.launch(mode, p, o, lse, again, ws, seed)
            torch.cuda.synchronize()
        except RuntimeError as e:
            if "hip" in str(e).lower():
                pytest.exit("%s: %s -- nothing more is launched on a device that reported an error" % (what, e), returncode=3)
            raise
        assert bool((ws[nws:] == 0xA5).all()), "%s: the backward wrote behind its %d-byte workspace" % (what, nws)
        og, dg, lg = o.fetch(what + " o"), dqkv.fetch(what + " dq/dk/dv"), lse.fetch(what + " lse").reshape(B, h, L)
        assert np.array_equal(dg.view(np.uint32), again.fetch(what + " second backward").view(np.uint32)), "%s: two backward calls differ" % what
        full = np.full((4, B * L, d), np.nan)                      # o, dq, dk, dv as [B, h, L, d_k], NaN at rows the layout does not hold
        full[:, self.sel] = np.stack([og, dg[:, :d], dg[:, d:2 * d], dg[:, 2 * d:]])
        return dict(zip(("o", "dq", "dk", "dv"), full.reshape(4, B, L, h, dk).transpose(0, 1, 3, 2, 4)), lse=lg.astype(np.float64))


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in CASES])
def test_xwide_attention_meets_the_entrywise_contract(c):
    X = A.Inputs(c)
    problems = [XwideProblem(c, X, layout) for layout in c.layouts]
    for p in c.pdrops:
        ref = X.reference(p)
        bars = {mode: A.bars(ref, X.q, X.k, X.v, X.do, mode) for mode in (1, 2)}
        for pr in problems:
            for mode in c.modes:
                pr.run(mode, p, ref, bars[mode], bars[1] if mode == 2 else None)
    for pr in problems:
        pr.inputs_unchanged()


def test_xwide_refusals_leave_the_outputs_untouched():
    LB, lib = _libs()
    B, L, h = 2, 40, 1
    mask, step = torch.zeros((B, L), dtype=torch.uint8, device=DEV), torch.full((1,), WORD, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    for what, kw, want in [("mode 0", dict(mode=0), EINVAL), ("d_k 128", dict(dk=128), EUNSUPPORTED), ("d_k 260", dict(dk=260), EUNSUPPORTED),
                           ("d_k 134", dict(dk=134), EUNSUPPORTED), ("NULL ws", dict(ws=None), EINVAL), ("p_drop 1", dict(p=1.0), EINVAL)]:
        kw = dict(dict(dk=256, mode=1, ws=ws, p=0.3), **kw)
        d = h * kw["dk"]
        rs, ors = (3 * d + 11) // 4 * 4, (d + 7) // 4 * 4
        qkv, dqkv = Win((B * L, 3 * d), rs, 4, GARBAGE, np.ones((B * L, 3 * d), np.float32)), Win((B * L, 3 * d), rs, 4, np.nan)
        o = Win((B * L, d), ors, 4, GARBAGE, np.ones((B * L, d), np.float32))
        lse = Win((1, B * h * L), B * h * L, 8, GARBAGE, np.ones((1, B * h * L), np.float32))
        at = lambda w: [w.ptr.value + 4 * d * j for j in range(3)]      # noqa: E731
        rest = (kw["p"], A.SEED, LB.ptr(step), None, None, kw["mode"])
        if kw["ws"] is not None:
            rc = lib.ltrx_mha_fwd_xwide(*at(qkv), LB.ptr(mask), B, L, h, kw["dk"], rs, o.ptr, ors, lse.ptr, *rest, LB.stream_of(ws))
            assert rc == want, "%s: the forward returned %d, expected %d" % (what, rc, want)
        rc = lib.ltrx_mha_bwd_xwide(*at(qkv), LB.ptr(mask), o.ptr, o.ptr, lse.ptr, B, L, h, kw["dk"], rs, ors, *at(dqkv), rs, *rest,
                                    LB.ptr(kw["ws"]), LB.stream_of(ws))
        assert rc == want, "%s: the backward returned %d, expected %d" % (what, rc, want)
        torch.cuda.synchronize()
        for w in (qkv, o, lse, dqkv):
            w.unchanged(what)
    assert not bool(ws.any()), "a refused backward wrote its workspace"
