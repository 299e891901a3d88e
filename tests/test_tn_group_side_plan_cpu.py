"""The host plan of ltrx_gemm_tn_group_ln's side job (no GPU): how many workgroups of the grouped weight-gradient launch run the
LayerNorm backward, which block of the stand-alone LayerNorm launch each of them plays, and when the side job is not taken
(ltrx_debug_tn_group_side_plan, include/ltrx.h)."""
import ctypes

import pytest

LAYER = [(1536, 512), (512, 512), (2048, 512), (512, 2048)]      # (NP, KP) of the four projections at d 512, d_ff 2048: 48 tiles


def _plan(lib, M, probs, rows, D, dres=1, side_wgs=0):
    n = len(probs)
    NP = (ctypes.c_int * n)(*[a for a, _ in probs])
    KP = (ctypes.c_int * n)(*[b for _, b in probs])
    gemm, vbl, owner = ctypes.c_int(-1), ctypes.c_int(-1), (ctypes.c_int * 320)()
    side = lib.ltrx_debug_tn_group_side_plan(n, M, NP, KP, rows, D, dres, side_wgs, ctypes.byref(gemm), ctypes.byref(vbl), owner)
    return side, gemm.value, vbl.value, list(owner)


@pytest.fixture(scope="module")
def lib():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("M,vblocks", [(256 * 240, 256), (64 * 240, 320)])
def test_bench_layer_gets_240_plus_16_workgroups(lib, M, vblocks):
    """both bench row counts: 48 tiles x 5 splits and 16 side workgroups, ids 240..255, two per XCD (workgroup w runs on XCD w % 8);
    every block of the LayerNorm launch (256 sixteen-wave blocks at 61440 rows, 320 four-wave blocks at 15360) has exactly one owner
    and side workgroup s owns s, s + 16, ..."""
    for dres in (1, 0):
        side, gemm, vbl, owner = _plan(lib, M, LAYER, M, 512, dres)
        assert (side, gemm, vbl) == (16, 240, vblocks)
        t_out, s_out = (ctypes.c_ubyte * 256)(), (ctypes.c_ubyte * 256)()
        NP = (ctypes.c_int * 4)(*[a for a, _ in LAYER])
        KP = (ctypes.c_int * 4)(*[b for _, b in LAYER])
        assert lib.ltrx_debug_tn_group_map(4, M, NP, KP, t_out, s_out) == gemm      # the GEMM path's ids are the map's
        ids = list(range(gemm, gemm + side))
        assert sorted(w % 8 for w in ids) == sorted(list(range(8)) * 2)
        assert all(o == -1 for o in owner[vbl:])
        assert sorted(set(owner[:vbl])) == ids
        for vb in range(vbl):
            assert owner[vb] == gemm + vb % side, (vb, owner[vb])
        per = [owner[:vbl].count(w) for w in ids]
        assert sum(per) == vbl and max(per) - min(per) <= (1 if vbl % side else 0)


def test_not_taken(lib):
    # the dropout composition of a layer's last launch: 16 tiles x 16 splits = 256 workgroups, no CU left over
    side, gemm, vbl, owner = _plan(lib, 256 * 240, [(512, 512), (1536, 512)], 256 * 240, 512)
    assert (side, gemm) == (0, 256) and all(o == -1 for o in owner)
    assert _plan(lib, 256 * 240, [(512, 512), (1536, 512)], 256 * 240, 512, side_wgs=4)[0] == 0
    # a row width outside the register-resident kernel (D % 256 != 0, D > 1024): the GEMM plan stands, no side job, forced or not
    for D in (384, 144, 1280):
        for force in (0, 16):
            side, gemm, vbl, owner = _plan(lib, 256 * 240, LAYER, 256 * 240, D, side_wgs=force)
            assert (side, gemm) == (0, 240) and all(o == -1 for o in owner), (D, force)
    # shapes on the per-problem path
    side, gemm, vbl, owner = _plan(lib, 4096, [(96, 136)], 4096, 512, side_wgs=8)
    assert (side, gemm) == (0, 0) and all(o == -1 for o in owner)
    # a LayerNorm far longer than the GEMM part: 8 K-steps per workgroup against 61440 rows to stream
    assert _plan(lib, 2048, [(256, 256)] * 4, 256 * 240, 512)[0] == 0


def test_forced_side_is_clamped_to_the_free_cus(lib):
    M = 256 * 240
    assert _plan(lib, M, LAYER, M, 512, side_wgs=1)[0] == 1
    assert _plan(lib, M, LAYER, M, 512, side_wgs=3)[0] == 3
    assert _plan(lib, M, LAYER, M, 512, side_wgs=16)[0] == 16
    assert _plan(lib, M, LAYER, M, 512, side_wgs=200)[0] == 16
    # one 256 x 256 problem, 160 rows... the large-tile kernel starts at 2048 rows: 2048 rows -> 16 splits of one tile, 240 CUs free
    side, gemm, vbl, owner = _plan(lib, 2048, [(256, 256)], 1056, 768, side_wgs=300)
    assert (side, gemm, vbl) == (240, 16, 66)
    assert [o for o in owner[:vbl]] == [16 + vb for vb in range(vbl)]     # more side workgroups than blocks: one block each
    side, gemm, vbl, owner = _plan(lib, 2048, [(256, 256)], 1056, 768, side_wgs=3)
    assert side == 3 and [o for o in owner[:vbl]] == [16 + vb % 3 for vb in range(vbl)]
    # invalid arguments: nothing taken
    assert _plan(lib, M, LAYER, M, 512, side_wgs=-1)[0] == 0
