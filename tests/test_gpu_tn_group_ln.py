"""-m gpu: ltrx_gemm_tn_group_ln -- the grouped weight-gradient launch with the LayerNorm backward as its side job -- against
ltrx_gemm_tn_group followed by ltrx_layernorm_bwd_partial on the same inputs, BIT FOR BIT: every dW and bias gradient, dx, the partial
rows [da | db] and their count.  dx and the partial-row workspace sit between NaN-filled guards that are checked afterwards.

Case axes: one 256 x 256 problem / four problems, one of them 512 x 256; row counts 32 (most virtual waves of the LayerNorm launch have
no row), 160 and 1056 (several rows per wave, ragged); D 256, 512, 768; with and without the residual gradient; 1, 3 and 16 forced side
workgroups, and the library's own choice.  The grouped kernel starts at 2048 GEMM rows (below that ltrx_gemm_tn_group itself runs one
ltrx_gemm_tn per problem and no side job exists), so every row count is run twice: as the row count of BOTH halves (the call's
fall-back: side_taken 0) and as the LayerNorm's row count next to a 2048-row GEMM (the side path: side_taken = the forced count).
LTRX_LN_BWD_WIDE_ROWS + 5 rows add the sixteen-wave launch shape the flagship step has (two passes of the eight waves)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_norm_head import _wide_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6
EINVAL = -1
GUARD = 1024                               # floats of sentinel before and after dx and the partial rows
WIDE_ROWS = _wide_rows()                   # LTRX_LN_BWD_WIDE_ROWS, read from csrc/ltrx_layernorm.hip
GEMM_ROWS = 2048                           # the smallest row count of the grouped kernel (tn256_ok)
ONE = [(256, 256)]
FOUR = [(256, 256), (512, 256), (256, 256), (256, 256)]


def _libs():
    from allrank_amd import _lib as LB
    return LB, LB.lib()


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_ok(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


class Inputs:
    def __init__(self, probs, M, rows, D):
        rng = np.random.default_rng(7 * M + 13 * rows + D + len(probs))
        t = lambda *s: torch.tensor(rng.standard_normal(s).astype(np.float32), device=DEV)
        self.probs, self.M, self.rows, self.D = probs, M, rows, D
        self.A = [t(M, a) for a, _ in probs]
        self.B = [t(M, b) for _, b in probs]
        self.dy, self.x, self.dres = t(rows, D), 3.0 * t(rows, D), t(rows, D)
        self.x[min(5, rows - 1)] = 1.25                                       # std = 0
        self.a = t(D)
        self.a[3] = 0.0
        LB, lib = _libs()
        b, y = t(D), torch.empty(rows, D, device=DEV)
        self.mean, self.rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
        P = LB.ptr
        LB.check(lib.ltrx_layernorm_fwd(P(self.x), None, P(self.a), P(b), rows, D, EPS, None, P(y), P(self.mean), P(self.rstd), 0.0, 0, None,
                                        None), "ln_fwd")
        n = len(probs)
        self.NP = (ctypes.c_int * n)(*[a for a, _ in probs])
        self.KP = (ctypes.c_int * n)(*[b for _, b in probs])
        nb = max(lib.ltrx_gemm_tn_group_workspace_bytes(n, M, self.NP, self.KP), 64)
        self.ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        self.ln_floats = max(lib.ltrx_layernorm_bwd_workspace_bytes(rows, D), 64) // 4
        self.keep = [v.clone() for v in self.A + self.B + [self.dy, self.x, self.dres, self.a, self.mean, self.rstd]]

    def untouched(self):
        return all(torch.equal(u, v) for u, v in zip(self.A + self.B + [self.dy, self.x, self.dres, self.a, self.mean, self.rstd], self.keep))

    def gemm_args(self, C, bias):
        n = len(self.probs)
        vp = ctypes.c_void_p * n
        return (n, vp(*[v.data_ptr() for v in self.A]), self.NP, vp(*[v.data_ptr() for v in self.B]), self.KP,
                vp(*[v.data_ptr() for v in C]), vp(*[v.data_ptr() for v in bias]), self.M, self.NP, self.KP, 0,
                ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel())

    def outputs(self):
        C = [torch.full((a, b), float("nan"), device=DEV) for a, b in self.probs]
        bias = [torch.full((a,), float("nan"), device=DEV) for a, _ in self.probs]
        return C, bias

    def reference(self, dres):
        """ltrx_gemm_tn_group, then ltrx_layernorm_bwd_partial"""
        LB, lib = _libs()
        P = LB.ptr
        C, bias = self.outputs()
        LB.check(lib.ltrx_gemm_tn_group(*self.gemm_args(C, bias), None, None, None, None), "gemm_tn_group")
        dx = torch.empty(self.rows, self.D, device=DEV)
        ws = torch.zeros(self.ln_floats, device=DEV)
        pr = ctypes.c_int(0)
        LB.check(lib.ltrx_layernorm_bwd_partial(P(self.dy), P(self.x), P(self.a), P(self.mean), P(self.rstd), P(self.dres) if dres else None,
                                                self.rows, self.D, EPS, P(dx), P(ws), ctypes.byref(pr), None), "ln_bwd_partial")
        torch.cuda.synchronize()
        return dict(C=C, bias=bias, dx=dx, partial=ws[:pr.value * 2 * self.D].clone(), rows=pr.value)

    def fused(self, dres, side_wgs):
        LB, lib = _libs()
        P = LB.ptr
        C, bias = self.outputs()
        dxb, dx = _guarded(self.rows * self.D)
        wsb, ws = _guarded(self.ln_floats)
        pr, taken = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = lib.ltrx_gemm_tn_group_ln(*self.gemm_args(C, bias), None, None, None, P(self.dy), P(self.x), P(self.a), P(self.mean),
                                       P(self.rstd), P(self.dres) if dres else None, self.rows, self.D, EPS, P(dx), P(ws),
                                       ctypes.byref(pr), side_wgs, ctypes.byref(taken), None)
        torch.cuda.synchronize()
        ok = _guards_ok(dxb, self.rows * self.D) and _guards_ok(wsb, self.ln_floats)
        return dict(rc=rc, C=C, bias=bias, dx=dx.view(self.rows, self.D), ws=ws, rows=pr.value, taken=taken.value, guards=ok)


def _same(got, ref, D, what):
    assert got["rc"] == 0, what
    assert got["guards"], "%s: wrote outside dx or the partial rows" % what
    assert got["rows"] == ref["rows"], what
    for p, (u, v) in enumerate(zip(got["C"], ref["C"])):
        assert torch.equal(u, v), "%s: dW of problem %d" % (what, p)
    for p, (u, v) in enumerate(zip(got["bias"], ref["bias"])):
        assert torch.equal(u, v), "%s: bias gradient of problem %d" % (what, p)
    assert torch.equal(got["dx"], ref["dx"]), "%s: dx" % what
    assert torch.equal(got["ws"][:ref["rows"] * 2 * D], ref["partial"]), "%s: partial rows" % what
    assert bool(torch.isnan(got["ws"][ref["rows"] * 2 * D:]).all()), "%s: wrote behind the partial rows" % what


def _free_cus(inp):
    _, lib = _libs()
    t_out, s_out = (ctypes.c_ubyte * 256)(), (ctypes.c_ubyte * 256)()
    nwg = lib.ltrx_debug_tn_group_map(len(inp.probs), inp.M, inp.NP, inp.KP, t_out, s_out)
    return 256 - nwg if nwg else 0


ROWS = [32, 160, 1056]
SHAPES = ([(probs, m, m, D) for probs in (ONE, FOUR) for m in ROWS for D in (256, 512, 768)]                # both halves on m rows
          + [(probs, GEMM_ROWS, m, D) for probs in (ONE, FOUR) for m in ROWS for D in (256, 512, 768)]     # the side path
          + [(FOUR, GEMM_ROWS, WIDE_ROWS + 5, 512), (ONE, GEMM_ROWS, WIDE_ROWS + 5, 256), (ONE, GEMM_ROWS, 1056, 1024)])


@pytest.mark.parametrize("probs,M,rows,D", SHAPES, ids=lambda v: str(len(v)) + "p" if isinstance(v, list) else str(v))
def test_forced_side_workgroups_give_the_two_launch_bits(probs, M, rows, D):
    inp = Inputs(probs, M, rows, D)
    free = _free_cus(inp)
    assert (free > 0) == (M >= GEMM_ROWS)
    for dres in (True, False):
        ref = inp.reference(dres)
        for side in (1, 3, 16):
            got = inp.fused(dres, side)
            _same(got, ref, D, "dres %s, side %d" % (dres, side))
            assert got["taken"] == min(side, free), (side, free, got["taken"])
    assert inp.untouched()


def test_the_librarys_own_choice():
    """side_wgs 0.  Taken: a 2048-row single-tile group (16 workgroups, 240 CUs free) next to a 160-row LayerNorm.  Not taken: next to
    a four-K-step GEMM part (five tiles x 16 splits, 2048 rows) 176 side workgroups would stream LTRX_LN_BWD_WIDE_ROWS + 5 rows of 512
    (134 MB) for longer than the GEMM part runs -- the call then is the two launches.  Also the deferred-reduction form: the slab pointers and split count ltrx_gemm_tn_group reports."""
    LB, lib = _libs()
    inp = Inputs(ONE, GEMM_ROWS, 160, 256)
    got = inp.fused(True, 0)
    _same(got, inp.reference(True), 256, "automatic, taken")
    assert got["taken"] == 240
    inp = Inputs(FOUR, GEMM_ROWS, WIDE_ROWS + 5, 512)
    assert _free_cus(inp) == 176
    got = inp.fused(True, 0)
    _same(got, inp.reference(True), 512, "automatic, not taken")
    assert got["taken"] == 0
    # deferred: same slabs, same split count, and the LayerNorm half as before
    P = LB.ptr
    n = len(inp.probs)
    vp = ctypes.c_void_p * n
    ref = inp.reference(False)
    C, bias = inp.outputs()
    so0, bso0, sp0 = vp(), vp(), ctypes.c_int(0)
    LB.check(lib.ltrx_gemm_tn_group(*inp.gemm_args(C, bias), so0, bso0, ctypes.byref(sp0), None), "gemm_tn_group(deferred)")
    torch.cuda.synchronize()
    nfl = inp.ws.numel() // 4
    slabs0 = inp.ws.view(torch.float32)[:nfl].clone()
    dxb, dx = _guarded(inp.rows * inp.D)
    wsb, ws = _guarded(inp.ln_floats)
    so1, bso1, sp1, pr, taken = vp(), vp(), ctypes.c_int(0), ctypes.c_int(-1), ctypes.c_int(-1)
    LB.check(lib.ltrx_gemm_tn_group_ln(*inp.gemm_args(C, bias), so1, bso1, ctypes.byref(sp1), P(inp.dy), P(inp.x), P(inp.a), P(inp.mean),
                                       P(inp.rstd), None, inp.rows, inp.D, EPS, P(dx), P(ws), ctypes.byref(pr), 1, ctypes.byref(taken),
                                       None), "gemm_tn_group_ln(deferred)")
    torch.cuda.synchronize()
    assert taken.value == 1 and sp1.value == sp0.value > 0 and list(so1) == list(so0) and list(bso1) == list(bso0)
    used = sum(sp0.value * a * b + ((sp0.value * a + 3) & ~3) for a, b in inp.probs)
    assert torch.equal(inp.ws.view(torch.float32)[:used], slabs0[:used])
    assert torch.equal(dx.view(inp.rows, inp.D), ref["dx"]) and pr.value == ref["rows"]
    assert torch.equal(ws[:pr.value * 2 * inp.D], ref["partial"])
    assert _guards_ok(dxb, inp.rows * inp.D) and _guards_ok(wsb, inp.ln_floats)


def test_aliasing_is_refused_and_nothing_is_launched():
    """dx or the partial rows inside an operand of the group: LTRX_EINVAL, every output still as it was"""
    LB, lib = _libs()
    P = LB.ptr
    D = 256
    inp = Inputs(FOUR, GEMM_ROWS, GEMM_ROWS, D)                    # A[0], B[0]: 2048 x 256, as large as dx
    lnws = torch.full((inp.ln_floats,), float("nan"), device=DEV)
    dx = torch.full((inp.rows, D), float("nan"), device=DEV)
    big = torch.zeros(inp.ln_floats + 64, device=DEV)
    for side in (0, 16):
        for what, dx_t, ws_t, A0, B0 in [("dx is A[0]", inp.A[0], lnws, None, None), ("dx is B[2]", inp.B[2], lnws, None, None),
                                         ("dx overlaps the tail of A[1]", None, lnws, "tail", None),
                                         ("partial rows inside B[0]", dx, None, None, big)]:
            C, bias = inp.outputs()
            args = list(inp.gemm_args(C, bias))
            n = len(inp.probs)
            vp = ctypes.c_void_p * n
            dx_ptr = dx_t.data_ptr() if dx_t is not None else inp.A[1].data_ptr() + 4 * (inp.A[1].numel() - 1)
            ws_ptr = ws_t.data_ptr() if ws_t is not None else big.data_ptr() + 64
            if B0 is not None:                                    # (B[0] := a buffer that holds the partial rows)
                bp = [v.data_ptr() for v in inp.B]
                bp[0] = B0.data_ptr()
                args[3] = vp(*bp)
            keep = [v.clone() for v in inp.A + inp.B]
            pr, taken = ctypes.c_int(-7), ctypes.c_int(-7)
            rc = lib.ltrx_gemm_tn_group_ln(*args, None, None, None, P(inp.dy), P(inp.x), P(inp.a), P(inp.mean), P(inp.rstd), P(inp.dres),
                                           inp.rows, D, EPS, ctypes.c_void_p(dx_ptr), ctypes.c_void_p(ws_ptr), ctypes.byref(pr), side,
                                           ctypes.byref(taken), None)
            torch.cuda.synchronize()
            assert rc == EINVAL, what
            assert taken.value == 0
            assert all(bool(torch.isnan(v).all()) for v in C + bias), what
            assert bool(torch.isnan(lnws).all()) and bool(torch.isnan(dx).all()) and not bool(big.any()), what
            assert all(torch.equal(u, v) for u, v in zip(inp.A + inp.B, keep)), what
