"""The contract of every dispatch arm of the split-bf16 GEMMs (allrank_amd/csrc/ltrx_gemm.hip), -m gpu.

One assertion everywhere, for EVERY entry (i, j), on operands that are not normalised and live in strided windows of larger buffers:

    |C_ij - epilogue64(emulated)_ij|  <=  ((P K + 3) 2^-24) (S_ij + |bias_j| + |residual_ij|)

`emulated` (tests/gemm_ref.py) is the fp64 sum of exactly the bf16 x bf16 products the kernel issues (P = 1, 3 or 6 per operand
pair), S = |A| |B|^T.  The right-hand side is the any-order bound of P K fp32 additions of exact products plus the bias, dropout-scale
and residual roundings: it contains no measured number, and with K <= 160 (K small for the six-product form) it is below the size
of one dropped cross term, so a kernel that loses a term, a fragment or a row stride fails it -- the next cheaper precision is shown
to fail it.  Around every window the buffers hold sentinels (NaN in outputs, large finite garbage in inputs) that must survive.
The worst error / bar of every case is logged as parity_gemm_contract.json, next to the other parity logs."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_ref as R
from tests.test_gpu_parity import DEV, _log, _t

pytestmark = pytest.mark.gpu

GARBAGE = np.float32(3.0e37)
EINVAL, EUNSUPPORTED = -1, -2
SEED, WORD = 77, 3
ROWS = []


def _libs():
    from allrank_amd import _lib as LB
    return LB, LB.lib()


class Win(object):
    """a [rows, cols] window with row stride ld, `off` floats into a larger device buffer filled with a sentinel"""

    def __init__(self, shape, ld, off=4, fill=np.nan, data=None):
        rows, cols = shape
        assert ld >= cols
        n = (off + rows * ld + 23) // 4 * 4
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, off
        self.host = np.full(n, fill, np.float32)
        if data is not None:
            self.view(self.host)[:] = data
        inside = np.zeros(n, bool)
        self.view(inside)[:] = True
        self.outside = ~inside
        self.dev = _t(self.host)
        self.ptr = ctypes.c_void_p(self.dev.data_ptr() + 4 * off)

    def view(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.off:], (self.rows, self.cols), (self.ld * flat.itemsize, flat.itemsize))

    def fetch(self, what):
        """the window after a call; everything outside it must hold its sentinel bit for bit"""
        now = self.dev.cpu().numpy()
        changed = (now.view(np.uint32) != self.host.view(np.uint32)) & self.outside
        assert not changed.any(), "%s: %d floats outside the [%d, %d] window (ld %d) were written, first at flat index %d" % (
            what, int(changed.sum()), self.rows, self.cols, self.ld, int(np.flatnonzero(changed)[0]) - self.off)
        return self.view(now).copy()

    def unchanged(self, what):
        now = self.dev.cpu().numpy()
        assert np.array_equal(now.view(np.uint32), self.host.view(np.uint32)), "%s: an input buffer was written" % what


def _contract(case, arm, got, out, pre, bar, zero_pattern):
    """the entrywise assertion (+ the zero pattern of ReLU / mask / dropout epilogues); logs and returns the worst error / bar"""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - out)
        ratio = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    i, j = (int(v) for v in np.unravel_index(int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio))), ratio.shape))
    worst = float(ratio[i, j])
    ROWS.append(dict(case=case, arm=arm, worst_error_over_bar=worst))
    assert worst <= 1.0, "%s [%s]: entry (%d, %d) is %r, reference %r, error %.4g against a bar of %.4g (ratio %.4g); %d of %d entries over" % (
        case, arm, i, j, float(got[i, j]), float(out[i, j]), float(err[i, j]), float(bar[i, j]), worst,
        int((~(ratio <= 1.0)).sum()), ratio.size)
    if zero_pattern:
        near = (np.abs(pre) <= bar) & (pre != 0)        # the sign of the pre-activation is not decided by the reference
        assert near.mean() <= 0.01, "%s [%s]: %d of %d pre-activations within the bar of 0" % (case, arm, int(near.sum()), near.size)
        bad = ((got == 0) != (out == 0)) & ~near
        assert not bad.any(), "%s [%s]: zero pattern differs at %d entries, first %s" % (case, arm, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    return worst


class NT(object):
    """one NT problem on the device: strided operand windows, cached emulations, and the call + check of one epilogue"""

    def __init__(self, case, rng, M, N, K, lda, ldb, scaled=True, offa=4, offb=4):
        self.case, self.M, self.N, self.K = case, M, N, K
        self.A, self.B = R.scaled_operands(rng, M, N, K, scaled)
        self.bias = (rng.standard_normal(N) * (2.0 ** rng.integers(-40, 41, N) if scaled else 1.0)).astype(np.float32)
        self.aux = (rng.standard_normal((M, N)) * (2.0 ** rng.integers(-20, 21, (M, 1)) if scaled else 1.0)).astype(np.float32)
        self.a = Win((M, K), lda, offa, GARBAGE, self.A)
        self.b = Win((N, K), ldb, offb, GARBAGE, self.B)
        self.step = torch.full((1,), WORD, dtype=torch.int32, device=DEV)
        self.S = R.abs_nt(self.A, self.B)
        self._em, self._img, self._wins = {}, None, {}

    def em(self, prec):
        if prec not in self._em:
            self._em[prec] = R.emulate_nt(self.A, self.B, prec)
        return self._em[prec]

    def image(self):
        LB, lib = _libs()
        if self._img is None:
            self._img = torch.empty_like(self.b.dev)
            LB.check(lib.ltrx_split_image(LB.ptr(self.b.dev), LB.ptr(self._img), self.b.dev.numel(), None), "split_image")
        return ctypes.c_void_p(self._img.data_ptr() + 4 * self.b.off)

    def win(self, kind, ld, off):
        key = (kind, ld, off)
        if key not in self._wins:
            if kind == "bias":
                self._wins[key] = Win((1, self.N), ld, off, GARBAGE, self.bias[None, :])
            else:
                self._wins[key] = Win((self.M, self.N), ld, off, GARBAGE, self.aux)
        return self._wins[key]

    def call(self, act, prec, tile, ldc, p=0.0, bias=True, ldaux=None, offc=4, offbias=4, offaux=4, image=False, inplace=False, rows=None):
        """one ltrx_gemm_nt call into a fresh NaN-filled C buffer; returns (rc, C window, C Win).  rows: (first, count) of A / C / aux"""
        LB, lib = _libs()
        r0, m = rows if rows else (0, self.M)
        ldaux = ldaux or self.N + 12
        if inplace:
            c = Win((self.M, self.N), ldc, offc, np.nan, self.aux)
            auxptr, ldaux = c.ptr, ldc
        else:
            c = Win((self.M, self.N), ldc, offc, np.nan)
            auxptr = self.win("aux", ldaux, offaux).ptr if act in (2, 3) else None
        bptr = self.win("bias", self.N, offbias).ptr if bias else None
        rc = lib.ltrx_gemm_nt(ctypes.c_void_p(self.a.ptr.value + 4 * r0 * self.a.ld), self.a.ld, self.b.ptr, self.b.ld,
                              self.image() if image else None, ctypes.c_void_p(c.ptr.value + 4 * r0 * ldc), ldc, m, self.N, self.K, bptr, act,
                              ctypes.c_void_p(auxptr.value + 4 * r0 * ldaux) if auxptr else None, ldaux if auxptr else 0,
                              p, SEED, LB.ptr(self.step) if p > 0 else None, prec, tile, None)
        return rc, c

    def expect(self, act, prec, p, bias):
        b = self.bias if bias else None
        out, pre = R.epilogue64(self.em(prec), act, b, self.aux if act in (2, 3) else None, p, SEED, WORD)
        bar = R.bar_nt(self.S, self.K, prec, b, self.aux if act == 3 else None)
        return out, pre, bar

    def run(self, arm, act, prec, tile, ldc, p=0.0, bias=True, **kw):
        """call + fetch (sentinels checked) + the contract; returns the C window"""
        LB, _ = _libs()
        tag = "%s act %d p %.2f prec %d tile %d ldc %d%s%s" % (self.case, act, p, prec, tile, ldc, " image" if kw.get("image") else "",
                                                               " in place" if kw.get("inplace") else "")
        rc, c = self.call(act, prec, tile, ldc, p, bias, **kw)
        LB.check(rc, tag)
        got = c.fetch(tag)
        out, pre, bar = self.expect(act, prec, p, bias)
        _contract(tag, arm, got, out, pre, bar, zero_pattern=(act in (1, 2) or p > 0) and act != 3)
        return got

    def inputs_unchanged(self):
        for w in [self.a, self.b] + list(self._wins.values()):
            w.unchanged(self.case)


EPILOGUES = [(0, 0.0), (1, 0.0), (2, 0.0), (3, 0.0), (0, 0.25), (1, 0.25), (2, 0.25), (3, 0.25)]
SMALL = [(1, 1, 4), (63, 127, 20), (64, 128, 36), (65, 130, 68), (129, 127, 136), (1, 128, 68), (63, 130, 136), (64, 1, 20),
         (65, 127, 4), (129, 128, 20), (129, 130, 36), (1, 127, 136), (63, 1, 36), (64, 130, 4), (65, 128, 136), (129, 1, 68)]


@pytest.mark.parametrize("prec", [0, 1, 2])
def test_small_tile_nt_every_epilogue_strided_and_scaled(prec):
    """the 128 x 128 x 32 kernel (tile 1 and the automatic choice) around its tile edges, every precision code, acts 0 .. 3 with and
    without dropout; ldc = N + 1 takes the scalar epilogue; one case with plain N(0, 1) operands, one dense"""
    for n, (M, N, K) in enumerate(SMALL):
        rng = np.random.default_rng(1000 + n)
        lda = K + (4 if n % 2 == 0 else 28)
        ldc = N + (4 if n % 3 else 1)
        if n == 5:
            lda, ldc = K, N
        nt = NT("small %dx%dx%d" % (M, N, K), rng, M, N, K, lda, K + 8 if n != 5 else K, scaled=(n != 3))
        for (act, p) in EPILOGUES:
            nt.run("nt128 prec %d" % prec, act, prec, n % 2, ldc, p, bias=(act != 2), ldaux=N + 12 if n != 5 else N)
        if K in (4, 20) and M * N >= 4096 and prec != 2:
            # the bar tells the precision codes apart: the next cheaper arithmetic fails it (CPU only)
            out, pre, bar = nt.expect(0, prec, 0.0, True)
            cheaper, _ = R.epilogue64(nt.em(2 if prec == 0 else 0), 0, nt.bias)
            assert (np.abs(cheaper - out) > bar).any(), (M, N, K, prec)
        nt.inputs_unchanged()
    _log("gemm_contract", ROWS)


@pytest.mark.parametrize("tile", [2, 3, 4])
def test_tile_codes_2_3_4_meet_the_reference(tile):
    """128x128x64, 256x128x32 and 256x128x64: K no multiple of 64, M ragged against 256"""
    for n, (M, N, K) in enumerate([(300, 130, 36), (257, 127, 96)]):
        rng = np.random.default_rng(2000 + 10 * tile + n)
        nt = NT("tile%d %dx%dx%d" % (tile, M, N, K), rng, M, N, K, K + 4, K + 8)
        for (act, p) in EPILOGUES:
            got = nt.run("nt tile %d" % tile, act, 0, tile, N + 4, p, bias=(act != 2))
            if act == 0:
                assert np.array_equal(got, nt.call(act, 0, 1, N + 4, p)[1].fetch("tile 1")), (tile, M, N, K)   # same summation order as tile 1
        nt.inputs_unchanged()
    _log("gemm_contract", ROWS)


LARGE = [(1, 256, 32), (63, 512, 96), (64, 256, 160), (65, 512, 32), (128, 256, 96), (129, 512, 160), (257, 256, 32), (300, 512, 96)]


@pytest.mark.parametrize("tile", [6, 7, 8])
def test_forced_large_tiles_every_epilogue(tile):
    """the 256 / 128 / 64-row forms of the 256-column kernel, forced: three- and one-product arithmetic, B read as fp32 and as
    the pre-split image, acts 0 .. 3 with and without dropout, act 3 in place"""
    for n, (M, N, K) in enumerate(LARGE):
        rng = np.random.default_rng(3000 + 10 * tile + n)
        nt = NT("large %dx%dx%d" % (M, N, K), rng, M, N, K, K + (4 if n % 2 else 28), K + 8, scaled=(n != 4))
        for prec in (0, 2):
            for image in (False, True):
                for (act, p) in EPILOGUES:
                    nt.run("nt256 tile %d prec %d" % (tile, prec), act, prec, tile, N + 4, p, bias=(act != 2), image=image)
                nt.run("nt256 tile %d prec %d" % (tile, prec), 3, prec, tile, N + 4, 0.25, image=image, inplace=True)
        if K == 32 and M >= 64:
            out, pre, bar = nt.expect(0, 0, 0.0, True)
            assert (np.abs(R.epilogue64(nt.em(2), 0, nt.bias)[0] - out) > bar).any(), (M, N, K)
        nt.inputs_unchanged()
    _log("gemm_contract", ROWS)


def _auto(case, seed, M, N, K, forced, epilogues, rows_split=None):
    """an automatic arm reached with a small M and a wide N: the contract, bit-equality with the forced tile it must have taken, and
    the library's own plan of the call (ltrx_debug_gemm_nt_plan) naming that tile, in the split case over exactly these row ranges"""
    rng = np.random.default_rng(seed)
    nt = NT(case, rng, M, N, K, K + 4, K + 8)
    plan = (ctypes.c_int * 14)()
    for (act, p) in epilogues:
        got = nt.run(case, act, 0, 0, N + 4, p, bias=(act != 2))
        # (the windows of this file start 16 bytes into their buffers and have leading dimensions % 4 == 0: aligned; no B image)
        nseg = _libs()[1].ltrx_debug_gemm_nt_plan(M, N, K, K + 4, K + 8, N + 4, act, int(act != 2), int(p > 0), 0, 0, 1, 0, plan)
        assert [tuple(plan[7 * i:7 * i + 3]) for i in range(nseg)] == (rows_split or [(0, M, forced)]), (case, act, p, list(plan))
        if rows_split is None:
            rc, c = nt.call(act, 0, forced, N + 4, p, bias=(act != 2))
            assert rc == 0 and np.array_equal(c.fetch(case).view(np.uint32), got.view(np.uint32)), (case, act, p)
        else:                      # two launches: each row range equals its own forced-tile call
            for (r0, m, f) in rows_split:
                rc, c = nt.call(act, 0, f, N + 4, p, bias=(act != 2), rows=(r0, m))
                assert rc == 0 and np.array_equal(c.fetch(case)[r0:r0 + m].view(np.uint32), got[r0:r0 + m].view(np.uint32)), (case, act, r0)
    nt.inputs_unchanged()
    _log("gemm_contract", ROWS)
    return nt


def test_auto_256_row_tile_at_168_to_256_tiles():
    _auto("auto v6 (168 tiles)", 4001, 33, 256 * 168, 32, 6, [(1, 0.25), (3, 0.0)])


def test_auto_256_row_tile_at_136_to_167_tiles():
    _auto("auto v6 (136 tiles, 272 of 128 rows)", 4002, 129, 256 * 136, 32, 6, [(0, 0.25), (2, 0.0)])


def test_auto_128_row_tile():
    _auto("auto v7 (176 tiles of 128 rows)", 4003, 129, 256 * 88, 32, 7, [(1, 0.0), (3, 0.25)])


def test_auto_64_row_tile():
    _auto("auto v8 (176 tiles of 64 rows)", 4004, 65, 256 * 88, 32, 8, [(2, 0.25), (0, 0.0)])


def test_auto_two_launch_row_split():
    """256 < tiles < 380: one round of 256-row tiles (m1 = 256 rows) and the remaining 44 rows as their own problem; acts 2 and 3 read
    aux, and every launch writes C, at row m1 of a stride that is not N"""
    N = 256 * 168                       # 336 tiles at M = 300; 168 in each launch: both take the 256-row tile
    _auto("auto split (336 tiles)", 4005, 300, N, 32, 6, [(2, 0.0), (3, 0.0), (2, 0.25)], rows_split=[(0, 256, 6), (256, 44, 6)])


def test_one_bit_relu_mask_epilogues_meet_the_reference():
    """acts 4 / 5 at the smallest tile count ltrx_gemm_nt_relu_bits_bytes accepts: against the reference of acts 1 / 2 (the mask of
    act 5 is the sign pattern of act 4's output, dropout included), not only against the kernels of acts 1 / 2"""
    LB, lib = _libs()
    M, N, K = 33, 256 * 168, 32
    assert lib.ltrx_gemm_nt_relu_bits_bytes(M, N, K) == 168 * 8192 and lib.ltrx_gemm_nt_relu_bits_bytes(M, N - 256, K) == 0
    rng = np.random.default_rng(4006)
    nt = NT("relu bits", rng, M, N, K, K + 4, K + 8)
    for p in (0.0, 0.25):
        bits = torch.zeros(168 * 8192 + 64, dtype=torch.uint8, device=DEV)
        bits[168 * 8192:] = 0xA5
        step = LB.ptr(nt.step) if p > 0 else None
        c = Win((M, N), N + 4, 4, np.nan)
        bias = nt.win("bias", N, 4)
        LB.check(lib.ltrx_gemm_nt(nt.a.ptr, nt.a.ld, nt.b.ptr, nt.b.ld, None, c.ptr, c.ld, M, N, K, bias.ptr, 4, LB.ptr(bits), 0, p, SEED, step, 0, 0, None), "act 4")
        fwd = c.fetch("act 4")
        out, pre, bar = nt.expect(1, 0, p, True)
        _contract("relu bits act 4 p %.2f" % p, "nt256 act 4", fwd, out, pre, bar, True)
        # backward over the same M, N: another A / B pair (the gradient and W2^T), the mask carried by the bits
        nt.aux = fwd                     # the saved activation acts 2 would read: same mask
        c2 = Win((M, N), N + 4, 4, np.nan)
        LB.check(lib.ltrx_gemm_nt(nt.a.ptr, nt.a.ld, nt.b.ptr, nt.b.ld, None, c2.ptr, c2.ld, M, N, K, None, 5, LB.ptr(bits), 0, p, SEED, step, 0, 0, None), "act 5")
        out, pre, bar = nt.expect(2, 0, p, False)
        _contract("relu bits act 5 p %.2f" % p, "nt256 act 5", c2.fetch("act 5"), out, pre, bar, True)
        assert bool((bits[168 * 8192:] == 0xA5).all())
    nt.inputs_unchanged()
    _log("gemm_contract", ROWS)


def test_unaligned_epilogue_pointers_take_the_small_tile():
    """C, bias or aux one float off 16-byte alignment (or ldc % 4 != 0): the automatic choice falls back to the 128 x 128 kernel and
    still meets the contract; a forced large tile refuses and leaves C alone"""
    M, N, K = 65, 256 * 88, 32          # aligned, this shape takes the 64-row large tile (test_auto_64_row_tile)
    rng = np.random.default_rng(4007)
    nt = NT("unaligned", rng, M, N, K, K + 4, K + 8)
    base = nt.call(3, 0, 1, N + 4, 0.0)[1].fetch("tile 1")
    for name, kw, ldc in [("C", dict(offc=5), N + 4), ("bias", dict(offbias=5), N + 4), ("aux", dict(offaux=5), N + 4), ("ldc", dict(), N + 1)]:
        got = nt.run("nt128 (unaligned %s)" % name, 3, 0, 0, ldc, 0.0, **kw)
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), name
        for tile in (6, 7, 8):
            rc, c = nt.call(3, 0, tile, ldc, 0.0, **kw)
            assert rc == EUNSUPPORTED, (name, tile, rc)
            assert np.isnan(c.fetch("refused")).all(), (name, tile)
    nt.inputs_unchanged()
    _log("gemm_contract", ROWS)


@pytest.mark.parametrize("tile", [1, 6, 7, 8])
def test_nt_non_finite_row_stays_in_its_row(tile):
    """one Inf / NaN in row m* of A: row m* of C is non-finite everywhere, every other row keeps its bits -- m* in the middle and as
    the last row of a ragged tile (300 = 256 + 44 = 2 * 128 + 44 = 4 * 64 + 44), where the large-tile kernels clamp their loads"""
    M, N, K = 300, 256, 96
    rng = np.random.default_rng(5000)
    nt = NT("nonfinite", rng, M, N, K, K + 4, K + 8)
    base = nt.call(0, 0, tile, N + 4)[1].fetch("base")
    assert np.isfinite(base).all()
    for bad in (np.inf, np.nan):
        for ms in (70, M - 1):
            A2 = nt.A.copy()
            A2[ms, 17] = bad
            a2 = Win((M, K), nt.a.ld, 4, GARBAGE, A2)
            saved, nt.a = nt.a, a2
            try:
                rc, c = nt.call(0, 0, tile, N + 4)
            finally:
                nt.a = saved
            got = c.fetch("nonfinite")
            assert rc == 0 and not np.isfinite(got[ms]).any(), (tile, bad, ms)
            keep = np.arange(M) != ms
            assert np.array_equal(got[keep].view(np.uint32), base[keep].view(np.uint32)), (tile, bad, ms)


def test_nt_argument_contract_refuses_and_leaves_c_alone():
    LB, lib = _libs()
    M, N, K = 64, 128, 36
    rng = np.random.default_rng(6000)
    nt = NT("args", rng, M, N, K, K + 4, K + 8)
    aux = nt.win("aux", N + 12, 4)

    def refused(want, what, lda=K + 4, ldb=K + 8, ldc=N + 4, k=K, act=0, ldaux=0, p=0.0, tile=0):
        c = Win((M, N), max(ldc, N), 4, np.nan)
        rc = lib.ltrx_gemm_nt(nt.a.ptr, lda, nt.b.ptr, ldb, None, c.ptr, ldc, M, N, k, None, act, aux.ptr if act in (2, 3) else None, ldaux,
                              p, SEED, None, 0, tile, None)
        assert rc == want, (what, rc)
        torch.cuda.synchronize()
        assert np.isnan(c.dev.cpu().numpy()).all(), what

    refused(EUNSUPPORTED, "K % 4", k=34)
    refused(EUNSUPPORTED, "lda % 4", lda=K + 2)
    refused(EUNSUPPORTED, "ldb % 4", ldb=K + 6)
    refused(EUNSUPPORTED, "lda < K", lda=K - 4)
    refused(EUNSUPPORTED, "ldc < N", ldc=N - 4)
    refused(EINVAL, "ldaux < N, act 2", act=2, ldaux=N - 4)
    refused(EINVAL, "ldaux < N, act 3", act=3, ldaux=N - 4)
    refused(EINVAL, "drop_p = 1", p=1.0)
    refused(EINVAL, "drop_p > 1", p=1.5)
    nt.inputs_unchanged()


# ---------------------------------------------------------------------------------------------------------------------------------
# TN: C[NP, KP] = A[M, NP]^T B[M, KP], bias_out = column sums of A
# ---------------------------------------------------------------------------------------------------------------------------------
class TN(object):
    def __init__(self, case, rng, M, NP, KP, lda, ldb, scaled=True):
        self.case, self.M, self.NP, self.KP = case, M, NP, KP
        At, Bt = R.scaled_operands(rng, NP, KP, M, scaled)          # the recipe on the transposes: the output rows / columns carry the 2^+-40
        self.A, self.B = np.ascontiguousarray(At.T), np.ascontiguousarray(Bt.T)
        self.a = Win((M, NP), lda, 4, GARBAGE, self.A)
        self.b = Win((M, KP), ldb, 4, GARBAGE, self.B)
        self.S = R.abs_tn(self.A, self.B)

    def call(self, prec, tile, want_bias=True, a=None):
        LB, lib = _libs()
        M, NP, KP = self.M, self.NP, self.KP
        c = Win((NP, KP), KP, 4, np.nan)
        gb = Win((1, NP), NP, 4, np.nan) if want_bias else None
        nbytes = lib.ltrx_gemm_tn_workspace_bytes(M, NP, KP)
        assert nbytes > 0
        ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=DEV)
        ws[nbytes:] = 0xA5
        rc = lib.ltrx_gemm_tn((a or self.a).ptr, self.a.ld, self.b.ptr, self.b.ld, c.ptr, gb.ptr if gb else None, M, NP, KP, prec, tile, LB.ptr(ws), None)
        tag = "%s prec %d tile %d" % (self.case, prec, tile)
        LB.check(rc, tag)
        got = c.fetch(tag)
        assert bool((ws[nbytes:] == 0xA5).all()), "%s: wrote past the %d workspace bytes" % (tag, nbytes)
        return got, (gb.fetch(tag)[0] if gb else None)

    def run(self, arm, prec, tile, want_bias=True):
        got, gb = self.call(prec, tile, want_bias)
        tag = "%s prec %d tile %d lda %d ldb %d" % (self.case, prec, tile, self.a.ld, self.b.ld)
        _contract(tag, arm, got, R.emulate_tn(self.A, self.B, prec), None, R.bar_tn(self.S, self.M, prec), False)
        if want_bias:
            ref = self.A.astype(np.float64).sum(0)
            _contract(tag + " bias", arm + " bias", gb[None, :], ref[None, :], None, R.bar_tn_bias(self.A, self.M)[None, :], False)
        self.a.unchanged(tag)
        self.b.unchanged(tag)
        return got, gb


@pytest.mark.parametrize("prec", [0, 1, 2])
def test_small_tile_tn_strided(prec):
    for n, (M, NP, KP) in enumerate([(1, 1, 1), (77, 5, 3), (129, 130, 36), (300, 128, 129)]):
        for (lda, ldb) in ((NP + 4, KP + 8), ((NP + 4) | 1, (KP + 8) | 1)):
            rng = np.random.default_rng(7000 + n)
            tn = TN("tn %dx%dx%d" % (M, NP, KP), rng, M, NP, KP, lda, ldb, scaled=(n != 1))
            got, _ = tn.run("tn128 prec %d" % prec, prec, 0, True)
            got2, _ = tn.run("tn128 prec %d" % prec, prec, 1, False)
            assert np.array_equal(got.view(np.uint32), got2.view(np.uint32))
            if prec == 0 and M == 129:       # the one-product sum fails the three-product bar (CPU only)
                assert (np.abs(R.emulate_tn(tn.A, tn.B, 2) - R.emulate_tn(tn.A, tn.B, 0)) > R.bar_tn(tn.S, M, 0)).any()
    _log("gemm_contract", ROWS)


@pytest.mark.parametrize("M,NP,KP,lda,ldb", [(2048, 256, 256, 256, 256), (2080, 256, 512, 256, 512), (2112, 256, 512, 256, 512),
                                              (2048, 512, 256, 516, 260)])
def test_large_tile_tn_at_its_smallest_shapes(M, NP, KP, lda, ldb):
    """the 256 x 256 split-K kernel: one tile, two tiles with 13 slabs of 160 rows (2080) and 14 slabs whose last holds 32 rows (2112),
    strided operands"""
    rng = np.random.default_rng(8000 + KP + NP + M)
    tn = TN("tn256 %dx%dx%d" % (M, NP, KP), rng, M, NP, KP, lda, ldb)
    for prec in (0, 2):
        tn.run("tn256 prec %d" % prec, prec, 0, True)
    tn.run("tn256 prec 0", 0, 0, False)
    _log("gemm_contract", ROWS)


@pytest.mark.parametrize("KP,ld", [(136, 256), (300, 512)])
def test_large_tile_tn_over_padded_rows(KP, ld):
    """tile 9: KP columns in rows of `ld` floats, garbage in the padding; C stays dense [NP, KP]"""
    rng = np.random.default_rng(8100 + KP)
    tn = TN("tn256 padded B %d in %d" % (KP, ld), rng, 2048, 256, KP, 260, ld)
    got, gb = tn.run("tn256 tile 9", 0, 9, True)
    _log("gemm_contract", ROWS)


@pytest.mark.parametrize("M,NP,KP,tile", [(300, 130, 36, 0), (2048, 256, 256, 0)])
def test_tn_non_finite_column_stays_in_its_row(M, NP, KP, tile):
    """one Inf / NaN in column n* of A touches row n* of C and bias_out[n*] only"""
    rng = np.random.default_rng(9000 + M)
    tn = TN("tn nonfinite", rng, M, NP, KP, NP + 4, KP + 8)
    base, gbase = tn.call(0, tile)
    assert np.isfinite(base).all() and np.isfinite(gbase).all()
    for bad in (np.inf, np.nan):
        for (m, ns) in ((M - 1, NP - 1), (37, 3)):
            A2 = tn.A.copy()
            A2[m, ns] = bad
            got, gb = tn.call(0, tile, a=Win((M, NP), tn.a.ld, 4, GARBAGE, A2))
            assert not np.isfinite(got[ns]).any() and not np.isfinite(gb[ns]), (bad, m, ns)
            keep = np.arange(NP) != ns
            assert np.array_equal(got[keep].view(np.uint32), base[keep].view(np.uint32)), (bad, m, ns)
            assert np.array_equal(gb[keep].view(np.uint32), gbase[keep].view(np.uint32)), (bad, m, ns)
