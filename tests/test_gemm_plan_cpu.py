"""The host-side launch plans of the GEMMs (allrank_amd/csrc/ltrx_gemm.hip: nt_plan, tn_plan, the grouped slab layout), no GPU.

Two independent statements of what the plans must be:
  * tests/golden/gemm_plan_parent.json -- what the planning exports returned at the commit named in the file, BEFORE the host code was
    rewritten around plans (tests/golden/make_gemm_plan_fixture.py): every value must still come out exactly;
  * tests/gemm_ref.py nt_plan_ref -- a transcription of that commit's ltrx_gemm_nt dispatch, which exported nothing: the plan hook
    (ltrx_debug_gemm_nt_plan) must agree with it exactly over the fixture's threshold-straddling shapes x every argument it reads.
"""
import ctypes
import itertools
import json
import os
import zlib

import pytest

from tests import gemm_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def rec():
    with open(os.path.join(HERE, "golden", "gemm_plan_parent.json")) as fh:
        return json.load(fh)


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _crc(buf, n):
    return zlib.crc32(bytes(bytearray(buf)[:n]))


def _nt_plan(lib, out, *args):
    n = lib.ltrx_debug_gemm_nt_plan(*(args + (out,)))
    return (0, [tuple(out[7 * i:7 * i + 7]) for i in range(n)]) if n else (out[0], [])


def _group_plan(lib, n, M, NP, KP, ws, lda=None, ldb=None, prec=0):
    splits, need = ctypes.c_int(-1), ctypes.c_size_t(0)
    took = lib.ltrx_debug_tn_group_plan(n, M, NP, KP, lda, ldb, prec, ws, ctypes.byref(splits), ctypes.byref(need))
    return took, splits.value, need.value


def test_fixture_covers_the_grid(rec):
    assert len(rec["commit"]) == 40 and rec["library_sources_modified"] is False
    assert 1000 <= len(rec["tn"]) + len(rec["relu_bits"]) + len(rec["groups"]) <= 5000
    tiles = {-(-M // 256) * (N // 256) for M, N, K, _ in rec["relu_bits"] if N % 256 == 0}
    for b in (136, 168, 176, 256, 360, 380):
        assert b - 1 in tiles and b in tiles and b + 1 in tiles, b
    rows = {M for M, _, _, _, _ in rec["tn"]}
    assert {2047, 2048, 2049, 2079, 2080, 2081, 2175, 2176, 2177, 15360, 61440} <= rows
    assert {(512, 136), (512, 46), (1536, 512), (512, 2048)} <= {(NP, KP) for _, NP, KP, _, _ in rec["tn"]}
    comps = {tuple(map(tuple, g["probs"])) for g in rec["groups"]}
    assert {((512, 2048), (2048, 512)), ((512, 512), (1536, 512))} <= comps           # the two-by-two dropout composition


def test_single_problem_tn_values_are_the_recorded_ones(lib, rec):
    sp, rps, kv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for M, NP, KP, splits, ws in rec["tn"]:
        assert lib.ltrx_gemm_tn_splits(M, NP, KP) == splits, (M, NP, KP)
        assert lib.ltrx_gemm_tn_workspace_bytes(M, NP, KP) == ws, (M, NP, KP)
        # the plan hook, dense operands, tile 0: the same split count, whole 32-row K-steps that cover M, and on the large tile (which
        # counts its splits after rounding the rows) no split without rows
        large = lib.ltrx_debug_gemm_tn_plan(M, NP, KP, NP, KP, 0, 0, ctypes.byref(sp), ctypes.byref(rps), ctypes.byref(kv))
        assert large == int(NP % 256 == 0 and KP % 256 == 0 and M % 32 == 0 and M >= 2048), (M, NP, KP)
        assert (sp.value, kv.value) == (splits, KP) and rps.value % 32 == 0 and M <= splits * rps.value, (M, NP, KP)
        assert not large or (splits - 1) * rps.value < M, (M, NP, KP)
        assert lib.ltrx_debug_gemm_tn_plan(M, NP, KP, NP, KP, 0, 1, ctypes.byref(sp), ctypes.byref(rps), ctypes.byref(kv)) == 0
        # every call the workspace was sized for fits it: weight slabs, then the bias rows (two per split on the small tile)
        assert (splits * NP * KP + 2 * splits * NP) * 4 <= ws, (M, NP, KP)


def test_padded_input_rows_take_the_large_tile_only_when_stated(lib):
    sp, rps, kv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    out = (ctypes.byref(sp), ctypes.byref(rps), ctypes.byref(kv))
    for F in (136, 46):
        for M in (61440, 15360):
            assert lib.ltrx_debug_gemm_tn_plan(M, 512, F, 512, 256, 0, 9, *out) == 1 and kv.value == F
            # one round of the 2 tiles of [512, 256]: 128 splits at most, each at least 128 rows
            assert sp.value == min(128, M // 128) and rps.value * sp.value >= M
            assert lib.ltrx_debug_gemm_tn_plan(M, 512, F, 512, 256, 2, 9, *out) == 1
            for (ldb, prec, tile) in [(256, 0, 0), (256, 1, 9), (F + (-F) % 4, 0, 9), (256, 0, 1)]:
                assert lib.ltrx_debug_gemm_tn_plan(M, 512, F, 512, ldb, prec, tile, *out) == 0, (F, M, ldb, prec, tile)
                assert sp.value == lib.ltrx_gemm_tn_splits(M, 512, F) and kv.value == F
    assert lib.ltrx_debug_gemm_tn_plan(4096, 512, 136, 511, 256, 0, 9, *out) == -1


def test_relu_bits_values_are_the_recorded_ones(lib, rec):
    for M, N, K, nbytes in rec["relu_bits"]:
        assert lib.ltrx_gemm_nt_relu_bits_bytes(M, N, K) == nbytes == R.relu_bits_bytes_ref(M, N, K), (M, N, K)


def test_grouped_values_are_the_recorded_ones(lib, rec):
    for g in rec["groups"]:
        n, M = len(g["probs"]), g["M"]
        NP, KP = _ints([a for a, _ in g["probs"]]), _ints([b for _, b in g["probs"]])
        assert lib.ltrx_gemm_tn_group_workspace_bytes(n, M, NP, KP) == g["ws_bytes"], g
        t_out, s_out = (ctypes.c_ubyte * 256)(), (ctypes.c_ubyte * 256)()
        wgs = lib.ltrx_debug_tn_group_map(n, M, NP, KP, t_out, s_out)
        assert (wgs, _crc(t_out, wgs), _crc(s_out, wgs)) == (g["wgs"], g["tile_crc"], g["split_crc"]), g
        for (rows, d, dres, sw, taken, gemm_wgs, vblocks, owner_crc) in g["side"]:
            gemm, vbl, owner = ctypes.c_int(-1), ctypes.c_int(-1), (ctypes.c_int * 320)()
            got = lib.ltrx_debug_tn_group_side_plan(n, M, NP, KP, rows, d, dres, sw, ctypes.byref(gemm), ctypes.byref(vbl), owner)
            assert (got, gemm.value, vbl.value, _crc(owner, 4 * 320)) == (taken, gemm_wgs, vblocks, owner_crc), (g["M"], g["probs"], rows, d)


def test_took_is_the_librarys_predicate(lib, rec):
    """FusedTrainer._wgrad_flush reports whether the grouped kernel ran.  With the workspace the engine allocates (the bound of the
    composition, or any larger one) the library's own decision equals the two-call expression the engine used before
    (ltrx_debug_tn_group_map(...) > 0 and ltrx_gemm_tn_group_workspace_bytes(...) <= ws); at the exact need it still groups, one byte
    below it does not.  The need is now compared exactly where it carried 4 floats of slack per problem: the recorded bound exceeds
    need + 16 bytes per problem everywhere, so no decision at a workspace sized by the library's own function moved."""
    largest = {}
    for g in rec["groups"]:
        largest[g["M"]] = max(largest.get(g["M"], 0), g["ws_bytes"])
    grouped = 0
    for g in rec["groups"]:
        n, M = len(g["probs"]), g["M"]
        NP, KP = _ints([a for a, _ in g["probs"]]), _ints([b for _, b in g["probs"]])
        old = g["wgs"] > 0                               # (and bound <= ws: true at both sizes below)
        for ws in (g["ws_bytes"], largest[M]):
            took, splits, need = _group_plan(lib, n, M, NP, KP, ws)
            assert bool(took) == old, (g, ws)
        if not old:
            assert (took, splits) == (0, 0), g
            continue
        grouped += 1
        total = sum((a // 256) * (b // 256) for a, b in g["probs"])
        assert splits * total == g["wgs"] and need == sum(splits * a * b + splits * a for a, b in g["probs"]) * 4, g
        assert need + 16 * n <= g["ws_bytes"], g
        assert _group_plan(lib, n, M, NP, KP, need)[:2] == (1, splits), g
        assert _group_plan(lib, n, M, NP, KP, need - 1)[:2] == (0, 0), g
        # what the exports above cannot see and the call applies: leading dimensions and the six-product precision
        assert _group_plan(lib, n, M, NP, KP, need, lda=NP, ldb=KP, prec=2)[0] == 1
        assert _group_plan(lib, n, M, NP, KP, need, prec=1)[0] == 0
        assert _group_plan(lib, n, M, NP, KP, need, lda=_ints([a + 2 for a in NP]), ldb=KP)[0] == 0
        assert _group_plan(lib, n, M, NP, KP, need, lda=NP, ldb=_ints([b - 4 for b in KP]))[0] == 0
    assert grouped >= 50


def _nt_shapes(rec, every=1):
    return [(M, N, K) for M, N, K, _ in rec["relu_bits"]][::every]


def test_nt_plan_is_the_transcribed_dispatch(lib, rec):
    """exact agreement with nt_plan_ref: the automatic choice over every shape x act x bias x dropout x precision x alignment x image,
    and every forced tile code 1..8 over a seventh of the shapes"""
    out = (ctypes.c_int * 14)()
    seen = {}
    opts = list(itertools.product(range(6), (0, 1), (0, 1), (0, 1, 2), (1, 0), (0, 1)))
    for (M, N, K) in _nt_shapes(rec):
        for (act, bias, drop, prec, vec, img) in opts:
            args = (M, N, K, K + 4, K + 8, N + 4, act, bias, drop, prec, 0, vec, img)
            got = _nt_plan(lib, out, *args)
            assert got == R.nt_plan_ref(*args), args
            for s in got[1]:
                seen[(len(got[1]),) + s[2:]] = seen.get((len(got[1]),) + s[2:], 0) + 1
    forced = list(itertools.product(range(1, 9), range(6), (0, 1), (0, 1, 2), (1, 0)))
    for (M, N, K) in _nt_shapes(rec, 7):
        for (tile, act, bias, prec, vec) in forced:
            args = (M, N, K, K, K, N, act, bias, 1 - bias, prec, tile, vec, bias)
            assert _nt_plan(lib, out, *args) == R.nt_plan_ref(*args), args
    # the sweep reached every automatic arm, in one launch and in the split window, and every epilogue kind
    tiles = {(k[0], k[1]) for k in seen}
    assert tiles >= {(1, 1), (1, 6), (1, 7), (1, 8), (2, 6), (2, 1), (2, 8)}, sorted(tiles)     # ((2, 7): the next test)
    assert {k[5] for k in seen} == set(range(6)) and {k[2] for k in seen} == {1, 2, 3}
    # refusals of the leading dimensions and K, whatever the tile
    for tile in (0, 1, 6):
        for (lda, ldb, ldc, K) in [(30, 32, 512, 32), (32, 28, 512, 32), (32, 32, 508, 32), (34, 32, 512, 32), (32, 38, 512, 32), (36, 36, 512, 34)]:
            args = (4096, 512, K, lda, ldb, ldc, 0, 1, 0, 0, tile, 1, 1)
            assert _nt_plan(lib, out, *args) == R.nt_plan_ref(*args) == (R.EUNSUPPORTED, []), args
    assert _nt_plan(lib, out, 0, 512, 32, 32, 32, 512, 0, 1, 0, 0, 0, 1, 1) == (-1, [])
    assert _nt_plan(lib, out, 256, 512, 32, 32, 32, 512, 6, 1, 0, 0, 0, 1, 1) == (-1, [])


def test_split_window_segments_choose_their_own_tile(lib):
    """both launches of the split window carry the automatic choice of their own rows.  N 130 tiles wide, 2 x 130 = 260 tiles: the first
    256 rows are 130 tiles of 256 rows or 260 of 128 -- neither large tile fills a round well, the small-tile kernel; N 100 tiles
    wide, 3 x 100 tiles: two rows of 256-row tiles first; the rest takes the 64-row, the 128-row or the small tile by its row count"""
    out = (ctypes.c_int * 14)()
    for (nn, m1, first, cases) in [(130, 256, 1, [(1, 1), (44, 1), (65, 8), (128, 8), (129, 1), (256, 1)]),
                                   (100, 512, 6, [(1, 1), (64, 1), (65, 8), (128, 8), (129, 7), (256, 7)])]:
        N = 256 * nn
        for (rest, second) in cases:
            args = (m1 + rest, N, 32, 32, 32, N, 0, 1, 0, 0, 0, 1, 1)
            rc, segs = _nt_plan(lib, out, *args)
            assert (rc, segs) == R.nt_plan_ref(*args)
            assert [s[:3] for s in segs] == [(0, m1, first), (m1, rest, second)], (nn, rest, segs)


def test_one_bit_mask_predicate_implies_one_256_row_segment(lib, rec):
    """wherever ltrx_gemm_nt_relu_bits_bytes is non-zero, the plan of act 4 and of act 5, dropout off and on, is ONE launch of the
    256-row tile: the (tile, thread) order the mask is kept in"""
    out = (ctypes.c_int * 14)()
    accepted = 0
    for (M, N, K) in _nt_shapes(rec):
        if lib.ltrx_gemm_nt_relu_bits_bytes(M, N, K) == 0:
            continue
        accepted += 1
        for (act, bias, drop, prec, img) in itertools.product((4, 5), (0, 1), (0, 1), (0, 2), (0, 1)):
            rc, segs = _nt_plan(lib, out, M, N, K, K, K + 4, N, act, bias, drop, prec, 0, 1, img)
            assert rc == 0 and len(segs) == 1 and segs[0][:3] == (0, M, 6), (M, N, K, act, bias, drop, prec, img, segs)
    assert accepted >= 100
