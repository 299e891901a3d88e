"""The contract of every attention kernel arm (allrank_amd/csrc/ltrx_mha.hip, ltrx_mha_res.hip), -m gpu.

One assertion for EVERY entry of O, lse, dQ, dK and dV, on inputs that are not normalised and live in strided windows of larger
buffers:  |kernel - fp64 reference| <= bar, with the reference, the derivation of the entrywise bars and the defect models in
tests/attention_ref.py.  tests/test_attention_ref_cpu.py is the evidence that the bars bite: plain fp32 attention stays below a
quarter of them on every case of the table, each defect model (a bf16-rounded operand, a skipped key tile, a missed rescale of the
lazy softmax reference, a wrong lse, another dropout mask in the backward, padded keys not zeroed, a head read too wide) is above
them.  Mode 2 (one bf16 product, outside the parity contract) meets the bars with its own product error and must fail mode 1's on O.
Around every window the buffers hold sentinels (NaN in outputs, 3e37 in inputs, a 4 KB tail behind a workspace of exactly
ltrx_mha_bwd_workspace_bytes) that must survive.  The worst error / bar of every (case, layout, arm, mode, p, tensor) is logged as
parity_attention_contract.json.

Which cases launch which instantiation (tests/attention_ref.py `instantiations`; test_attention_ref_cpu.py asserts that none of the
36 is left out, this file asserts the backward arm of every call against ltrx_mha_bwd_workspace_bytes):

  ltrx_mha_{fwd,bwd_dq,bwd_dkdv}_kernel<32, DROP=0/1>    exact dk4 L33; exact dk32 L129; mask * exact            (p 0 / p 0.3)
  ltrx_mha_{fwd,bwd_dq,bwd_dkdv}_kernel<64, DROP=0/1>    exact dk64 L161; climbing (mode 0)
  ltrx_mha_{bwd_dq,bwd_dkdv}_kernel<64, DROP=0/1>        also mixed L2049, mixed budget (after the resident forward, modes 1 / 2)
  ltrx_mha_{fwd,bwd_dq,bwd_dkdv}_kernel<96, DROP=0/1>    exact dk68 L130; exact dk96 L130                        (p 0 / p 0.1)
  ltrx_mha_{fwd,bwd_dq,bwd_dkdv}_kernel<128, DROP=0/1>   exact dk100 L70; exact dk124 L70; exact dk128 L33
  ltrx_mha_fwd_res_kernel<DROP=0/1, PL=0>                resident dk36/60/64 ragged256/ragged289; mask * resident; climbing; mixed * (mode 1)
  ltrx_mha_fwd_res_kernel<DROP=0/1, PL=1>                resident dk36/60/64 ragged256/ragged289; mixed * (mode 2)
  ltrx_mha_bwd_dkdv_res_kernel<DROP=0/1, PL=0>           resident dk36/60/64 ragged256/ragged289; mask * resident; climbing (mode 1)
  ltrx_mha_bwd_dkdv_res_kernel<DROP=0/1, PL=1>           resident dk36/60/64 ragged256/ragged289 (mode 2)
  ltrx_mha_bwd_dq_res_kernel<PL=0, NW=4>                 resident dk36/60/64 ragged256; mask * resident; climbing
  ltrx_mha_bwd_dq_res_kernel<PL=1, NW=4>                 resident dk36/60/64 ragged256 (mode 2)
  ltrx_mha_bwd_dq_res_kernel<PL=0/1, NW=8>               resident dk36/60/64 ragged289 (modes 1 / 2)
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import attention_ref as A
from tests.test_gpu_gemm_contract import GARBAGE, Win
from tests.test_gpu_parity import DEV, _log

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
WORD = 3
TAIL = 4096
ROWS = []
CONSTS = A.header_constants()


def _libs():
    from allrank_amd import _lib as LB
    return LB, LB.lib()


def _rows2d(x):
    """[B, h, L, d_k] -> [B L, h d_k]: element (b, l, head, c) at ((b L + l) h + head) d_k + c"""
    B, h, L, dk = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B * L, h * dk)


class Problem(object):
    """one case on the device in one layout: input windows (shared by every mode and dropout rate), and the call + check of one
    (mode, p_drop)"""

    def __init__(self, c, X, layout):
        self.c, self.X, self.layout = c, X, layout
        B, h, L, dk = c.B, c.h, c.L, c.dk
        d = h * dk
        self.d = d
        self.rs, self.ors, self.drs = (3 * d + 8, d + 4, 3 * d + 12) if c.strides == "own" else (3 * d, d, 3 * d)
        if layout == "cu":
            assert X.lens is not None
            self.sel = ~X.mask.reshape(-1)                                     # packed rows: the valid items of every slate
            cu = np.zeros(B + 1, np.int32)
            cu[1:] = np.cumsum(X.lens)
            self.cu = torch.tensor(cu, device=DEV)
            order = np.argsort(-np.asarray(X.lens), kind="stable").astype(np.int32)                  # longest first, as the engine launches
            if np.array_equal(order, np.arange(B)):
                order = order[::-1].copy()                                                         # never the identity
            self.order = torch.tensor(order, device=DEV)
            self.mask = None
        else:
            self.sel = np.ones(B * L, bool)
            self.cu = None
            self.order = torch.tensor(np.arange(B)[::-1].astype(np.int32).copy(), device=DEV) if B <= 8 else None
            self.mask = torch.tensor(X.mask.astype(np.uint8), device=DEV)
        self.R = int(self.sel.sum())
        qkv = np.concatenate([_rows2d(X.q), _rows2d(X.k), _rows2d(X.v)], 1)[self.sel]
        self.qkv = Win((self.R, 3 * d), self.rs, 4, GARBAGE, qkv)
        self.do = Win((self.R, d), self.ors, 4, GARBAGE, _rows2d(X.do)[self.sel])
        self.step = torch.full((1,), WORD, dtype=torch.int32, device=DEV)
        self.tag = "%s [%s, %s strides]" % (c.name, layout, c.strides)

    def _p(self, win, col=0):
        return ctypes.c_void_p(win.ptr.value + 4 * col)

    def call(self, mode, p, seed=A.SEED):
        """forward + backward into fresh NaN-filled windows; returns {tensor: [B, h, L, ..] array, NaN where the layout holds no row}"""
        LB, lib = _libs()
        c, d = self.c, self.d
        B, h, L, dk = c.B, c.h, c.L, c.dk
        what = "%s mode %d p %g" % (self.tag, mode, p)
        o = Win((self.R, d), self.ors, 4, np.nan)
        lse = Win((1, B * h * L), B * h * L, 8, np.nan)
        dqkv = Win((self.R, 3 * d), self.drs, 4, np.nan)
        nws = lib.ltrx_mha_bwd_workspace_bytes(B, L, h, dk, mode)
        assert nws == A.bwd_workspace_bytes(mode, B, L, h, dk, CONSTS), "%s: the backward arm is not the one the case is meant for" % what
        ws = torch.full((nws + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
        q, k, v = self._p(self.qkv), self._p(self.qkv, d), self._p(self.qkv, 2 * d)
        st = LB.stream_of(ws)
        try:
            LB.check(lib.ltrx_mha_fwd(q, k, v, LB.ptr(self.mask), B, L, h, dk, self.rs, o.ptr, self.ors, lse.ptr, p, seed, LB.ptr(self.step),
                                      LB.ptr(self.cu), LB.ptr(self.order), mode, st), what + " fwd")
            LB.check(lib.ltrx_mha_bwd(q, k, v, LB.ptr(self.mask), o.ptr, self.do.ptr, lse.ptr, B, L, h, dk, self.rs, self.ors,
                                      self._p(dqkv), self._p(dqkv, d), self._p(dqkv, 2 * d), self.drs, p, seed, LB.ptr(self.step),
                                      LB.ptr(self.cu), LB.ptr(self.order), mode, LB.ptr(ws), st), what + " bwd")
            torch.cuda.synchronize()
        except RuntimeError as e:
            if "HIP error" in str(e) or "hip" in str(e).lower():
                pytest.exit("%s: %s -- nothing more is launched on a device that reported an error" % (what, e), returncode=3)
            raise
        assert bool((ws[nws:] == 0xA5).all()), "%s: the backward wrote behind its %d-byte workspace" % (what, nws)
        og, dg, lg = o.fetch(what + " o"), dqkv.fetch(what + " dq/dk/dv"), lse.fetch(what + " lse").reshape(B, h, L)

        def heads(rows2d):
            full = np.full((B * L, d), np.nan)
            full[self.sel] = rows2d
            return full.reshape(B, L, h, dk).transpose(0, 2, 1, 3)

        return dict(o=heads(og), lse=lg.astype(np.float64), dq=heads(dg[:, :d]), dk=heads(dg[:, d:2 * d]), dv=heads(dg[:, 2 * d:]))

    def compared(self, t):
        """[B, 1 or h, L(, 1)] rows the layout holds: all in the padded layout, a slate's first len rows in the packed one"""
        rows = self.sel.reshape(self.c.B, 1, self.c.L)
        return rows if t == "lse" else rows[..., None]

    def ratios(self, got, ref, bar):
        """{tensor: (worst error / bar, index, error, bar)} over the rows the layout holds; the others must still be NaN"""
        out = {}
        for t in A.TENSORS:
            rows = np.broadcast_to(self.compared(t), got[t].shape)
            assert np.isnan(got[t][~rows]).all(), "%s: %s has values at rows beyond a slate's length" % (self.tag, t)
            out[t] = A.worst(np.where(rows, got[t], getattr(ref, t)), getattr(ref, t), bar[t])
        return out

    def run(self, mode, p, ref, bar, bar1=None):
        c = self.c
        arm = A.arm_name(mode, c.B, c.L, c.h, c.dk, CONSTS)
        got = self.call(mode, p)
        res = self.ratios(got, ref, bar)
        for t in A.TENSORS:
            ROWS.append(dict(case=c.name, layout=self.layout, strides=c.strides, arm=arm, mode=mode, p_drop=p, tensor=t,
                             worst_error_over_bar=res[t][0]))
        for t in A.TENSORS:
            ratio, idx, err, b = res[t]
            assert ratio <= 1.0, "%s, %s arm, mode %d, p %g: %s at (slate, head, row%s) = %s is %r, reference %r, error %.4g against a bar of %.4g (ratio %.4g)" % (
                self.tag, arm, mode, p, t, "" if t == "lse" else ", col", idx, float(got[t][idx]), float(getattr(ref, t)[idx]), err, b, ratio)
        if self.layout == "padded":                      # padded keys: exactly 0 in dK and dV (their bar is 0, too)
            pad = np.broadcast_to(self.X.mask[:, None, :, None], got["dk"].shape)
            assert (got["dk"][pad] == 0).all() and (got["dv"][pad] == 0).all(), self.tag
            for b in np.flatnonzero(self.X.mask.all(-1)):    # a fully padded slate: all five outputs exactly 0
                for t in A.TENSORS:
                    assert (got[t][b] == 0).all(), "%s: %s of the fully padded slate %d is not 0" % (self.tag, t, b)
        if bar1 is not None:                             # mode 2: one product per contraction must not pass for three
            r1 = self.ratios(got, ref, bar1)["o"][0]
            ROWS.append(dict(case=c.name, layout=self.layout, strides=c.strides, arm=arm, mode=mode, p_drop=p, tensor="o against the mode-1 bar",
                             worst_error_over_bar=r1))
            assert r1 > 1.0, "%s mode 2, p %g: O meets the bar of mode 1 (ratio %.4g): the case does not tell one bf16 product from three" % (self.tag, p, r1)
        return got

    def inputs_unchanged(self):
        self.qkv.unchanged(self.tag + " q/k/v")
        self.do.unchanged(self.tag + " dO")
        if self.mask is not None:
            assert np.array_equal(self.mask.cpu().numpy(), self.X.mask.astype(np.uint8)), self.tag


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in A.CASES])
def test_attention_arm_meets_the_entrywise_contract(c):
    X = A.Inputs(c)
    problems = [Problem(c, X, layout) for layout in c.layouts]
    for p in c.pdrops:
        ref = X.reference(p)
        bars = {mode: A.bars(ref, X.q, X.k, X.v, X.do, mode) for mode in sorted(set(c.modes) | ({1} if 2 in c.modes else set()))}
        for pr in problems:
            for mode in c.modes:
                pr.run(mode, p, ref, bars[mode], bars[1] if mode == 2 else None)
    for pr in problems:
        pr.inputs_unchanged()
    _log("attention_contract", ROWS)


@pytest.mark.parametrize("name,mode,p", [("resident dk64 ragged256", 1, 0.3), ("exact dk96 L130", 0, 0.1)])
def test_forward_and_backward_regenerate_the_oracles_keep_mask(name, mode, p):
    """the kernels' keep pattern is the oracle's: against the reference under the SAME seed the contract holds (the test above);
    against the reference under seed + 1 -- another zero pattern, in the forward or in the backward alone -- the same outputs fail it"""
    c = [c for c in A.CASES if c.name == name][0]
    X = A.Inputs(c)
    got = Problem(c, X, "padded").call(mode, p)
    ref = X.reference(p)
    res = {t: A.worst(got[t], getattr(ref, t), A.bars(ref, X.q, X.k, X.v, X.do, mode)[t])[0] for t in A.TENSORS}
    assert max(res.values()) <= 1.0, res
    other = A.reference(X.q, X.k, X.v, X.do, X.mask, X.keep(p, A.SEED + 1))
    bar = A.bars(other, X.q, X.k, X.v, X.do, mode)
    assert A.worst(got["o"], other.o, bar["o"])[0] > 1.0 and A.worst(got["dv"], other.dv, bar["dv"])[0] > 1.0
    mixed = A.variant(X.q, X.k, X.v, X.do, X.mask, X.keep(p), keep_bwd=X.keep(p, A.SEED + 1))     # forward right, backward wrong
    bar = A.bars(ref, X.q, X.k, X.v, X.do, mode)
    assert A.worst(got["o"], mixed["o"], bar["o"])[0] <= 1.0
    assert max(A.worst(got[t], mixed[t], bar[t])[0] for t in ("dq", "dk", "dv")) > 1.0


def test_refusals_leave_the_outputs_untouched():
    LB, lib = _libs()
    B, L, h = 2, 40, 2
    mask = torch.zeros((B, L), dtype=torch.uint8, device=DEV)
    step = torch.full((1,), WORD, dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, L, 2 * L], dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    st = LB.stream_of(ws)
    nan = float("nan")
    cases = [("d_k 6", dict(dk=6), EUNSUPPORTED), ("d_k 132", dict(dk=132), EUNSUPPORTED),
             ("row stride below h d_k", dict(rs=60), EUNSUPPORTED), ("row stride no multiple of 4", dict(rs=198), EUNSUPPORTED),
             ("o stride below h d_k", dict(ors=60), EUNSUPPORTED), ("o stride no multiple of 4", dict(ors=66), EUNSUPPORTED),
             ("d stride below h d_k", dict(drs=60), EUNSUPPORTED, "bwd"), ("d stride no multiple of 4", dict(drs=198), EUNSUPPORTED, "bwd"),
             ("mode 3", dict(mode=3), EINVAL), ("mode -1", dict(mode=-1), EINVAL), ("p_drop 1", dict(p=1.0), EINVAL),
             ("p_drop NaN", dict(p=nan), EINVAL), ("p_drop < 0", dict(p=-0.1), EINVAL),
             ("neither mask nor cu_seqlens", dict(mask=None), EINVAL)]
    for mode in (0, 1):
        for case in cases:
            what, kw, want = case[0], dict(dk=32 if mode == 0 else 64, rs=None, ors=None, drs=None, mode=mode, p=0.3, mask=mask), case[2]
            kw.update(case[1])
            dk = kw["dk"]
            d = h * dk
            rs, ors, drs = kw["rs"] or 3 * d + 8, kw["ors"] or d + 4, kw["drs"] or 3 * d + 12
            ld = max(3 * d + 12, rs, drs)
            qkv = Win((B * L, ld), ld, 4, GARBAGE, np.ones((B * L, ld), np.float32))
            o = Win((B * L, ld), ld, 4, np.nan)
            lse = Win((1, B * h * L), B * h * L, 8, np.nan)
            dqkv = Win((B * L, ld), ld, 4, np.nan)
            ptr = lambda w, col=0: ctypes.c_void_p(w.ptr.value + 4 * col)      # noqa: E731
            if len(case) == 3:
                rc = lib.ltrx_mha_fwd(ptr(qkv), ptr(qkv, d), ptr(qkv, 2 * d), LB.ptr(kw["mask"]), B, L, h, dk, rs, o.ptr, ors, lse.ptr, kw["p"],
                                      A.SEED, LB.ptr(step), None, None, kw["mode"], st)
                assert rc == want, "forward, %s (mode %d): returned %d, expected %d" % (what, mode, rc, want)
            rc = lib.ltrx_mha_bwd(ptr(qkv), ptr(qkv, d), ptr(qkv, 2 * d), LB.ptr(kw["mask"]), o.ptr, o.ptr, lse.ptr, B, L, h, dk, rs, ors,
                                  ptr(dqkv), ptr(dqkv, d), ptr(dqkv, 2 * d), drs, kw["p"], A.SEED, LB.ptr(step), None, None, kw["mode"],
                                  LB.ptr(ws), st)
            assert rc == want, "backward, %s (mode %d): returned %d, expected %d" % (what, mode, rc, want)
            torch.cuda.synchronize()
            for w in (qkv, o, lse, dqkv):
                w.unchanged("%s (mode %d)" % (what, mode))
    assert not bool(ws.any()), "a refused backward wrote its workspace"
    # (the packed layout needs no mask: accepted)
    d = h * 32
    qkv = Win((B * L, 3 * d), 3 * d, 4, GARBAGE, np.ones((B * L, 3 * d), np.float32))
    o = Win((B * L, d), d, 4, np.nan)
    lse = Win((1, B * h * L), B * h * L, 8, np.nan)
    LB.check(lib.ltrx_mha_fwd(qkv.ptr, ctypes.c_void_p(qkv.ptr.value + 4 * d), ctypes.c_void_p(qkv.ptr.value + 8 * d), None, B, L, h, 32, 3 * d,
                              o.ptr, d, lse.ptr, 0.0, A.SEED, None, LB.ptr(cu), None, 0, st), "packed layout without a mask")
    assert np.isfinite(o.fetch("o")).all()
