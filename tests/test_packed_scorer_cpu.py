"""Host logic of the packed validation scorer (engine.FusedScorer): the row-bucket ladder, the host half of the batch stager, and
the argument checks of the device-count pack / unpack entry points (returned before any HIP call, so this runs without a GPU)."""
import ctypes

import pytest
import torch

from allrank_amd.engine import row_bucket, _stage_host


def test_row_bucket_ladder():
    rungs = sorted({row_bucket(n) for n in range(1, 200000)})
    assert rungs[:8] == [32, 64, 96, 128, 160, 192, 224, 256]
    assert all(r % 32 == 0 for r in rungs)
    assert all(b > a for a, b in zip(rungs, rungs[1:]))
    assert all(b - a <= max(32, a // 8) for a, b in zip(rungs, rungs[1:]))          # at most 1/8 above the rung below from 256 on
    prev = 0
    for n in list(range(1, 5000)) + list(range(5000, 400000, 997)):
        b = row_bucket(n)
        assert n <= b < n + max(32, n / 8.0) and b >= prev, n                        # monotone, slack < 32 rows or < n/8
        prev = b
    assert row_bucket(0) == 32
    assert row_bucket(10 ** 6, cap=4096) == 4096 and row_bucket(100, cap=4096) == 128


def test_stage_host_layout():
    """[ids as int32 pairs, 2B |] cu_seqlens [B+1], stable longest-first order [B]; missing slates count as length 0 / id 0"""
    B, lens, ids = 5, [3, 0, 7, 7, 1], [9, 2, 4, 4, 0]
    host = torch.full((4 * B + 1,), -7, dtype=torch.int32)
    assert _stage_host(host, B, lens, ids) == 18
    assert host[:2 * B].view(torch.int64).tolist() == ids                            # the ids: an int64 view at offset 0
    assert host[2 * B:3 * B + 1].tolist() == [0, 3, 3, 10, 17, 18]
    assert host[3 * B + 1:].tolist() == [2, 3, 0, 4, 1]                              # ties keep their original order
    host.fill_(-7)
    assert _stage_host(host, B, lens[:3], ids[:3]) == 10                             # only 3 slates given: the rest length 0, id 0
    assert host[:2 * B].view(torch.int64).tolist() == [9, 2, 4, 0, 0]
    assert host[2 * B:3 * B + 1].tolist() == [0, 3, 3, 10, 10, 10]
    assert host[3 * B + 1:].tolist() == [2, 0, 1, 3, 4]
    host = torch.full((2 * B + 1,), -7, dtype=torch.int32)                           # without ids: cu then order
    assert _stage_host(host, B, lens) == 18
    assert host[:B + 1].tolist() == [0, 3, 3, 10, 17, 18] and host[B + 1:].tolist() == [2, 3, 0, 4, 1]


@pytest.fixture(scope="module")
def lib():
    from allrank_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_packed_entry_points_reject_bad_arguments(lib):
    f = ctypes.c_void_p(4096)                         # never dereferenced: every check comes before a launch
    ok = dict(B=4, L=16, F=8, rows=64, ld=8)

    def assemble(**kw):
        a = dict(ok, **kw)
        ptrs = kw.get("ptrs", [f] * 5)
        return lib.ltrx_assemble_packed(*ptrs, a["B"], a["L"], a["F"], a["rows"], kw.get("x_out", f), a["ld"], kw.get("y_out", f),
                                        None, None, None)
    for bad in ([None, f, f, f, f], [f, None, f, f, f], [f, f, None, f, f], [f, f, f, None, f], [f, f, f, f, None]):
        assert assemble(ptrs=bad) == -1
    assert assemble(x_out=None) == -1 and assemble(y_out=None) == -1
    assert assemble(B=0) == -1 and assemble(L=0) == -1 and assemble(F=0) == -1 and assemble(rows=-1) == -1 and assemble(ld=7) == -1
    assert assemble(B=1 << 16, L=1 << 16) == -1                   # B * L beyond int32 (the packed -> grid index is int32)

    def gather(src=f, cu=f, dst=f, B=4, L=16, cols=8, rows=64, ld_src=8, ld_dst=8):
        return lib.ltrx_gather_rows_cu(src, ld_src, cu, B, L, cols, rows, dst, ld_dst, None, None)
    assert gather(src=None) == -1 and gather(cu=None) == -1 and gather(dst=None) == -1
    assert gather(B=0) == -1 and gather(L=-1) == -1 and gather(cols=0) == -1 and gather(rows=-1) == -1
    assert gather(ld_src=7) == -1 and gather(ld_dst=7) == -1
    assert gather(rows=0) == 0                                    # nothing to launch

    def scatter(src=f, cu=f, dst=f, B=4, L=16, cols=1, rows=64, ld_src=1, ld_dst=1):
        return lib.ltrx_scatter_rows_cu(src, ld_src, cu, B, L, cols, rows, dst, ld_dst, None)
    assert scatter(src=None) == -1 and scatter(cu=None) == -1 and scatter(dst=None) == -1
    assert scatter(B=0) == -1 and scatter(L=0) == -1 and scatter(cols=0) == -1 and scatter(rows=-1) == -1
    assert scatter(cols=3, ld_src=2) == -1 and scatter(cols=3, ld_src=3, ld_dst=2) == -1
