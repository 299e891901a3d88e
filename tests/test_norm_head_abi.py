"""No GPU: the fused final-norm + score-head entry points are built for gfx950, exported, bound from the header, and refuse what
they do not take before any launch (the argument checks run on the host: no pointer is dereferenced)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from allrank_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_prototypes_come_from_the_header(lib):
    from allrank_amd import _lib
    assert _lib.PROTOTYPES["ltrx_norm_head_fwd"] == ("int", ["*"] * 5 + ["int", "int", "float"] + ["*"] * 4 + ["ltrx_stream_t"])
    assert _lib.PROTOTYPES["ltrx_norm_head_bwd_partial"] == ("int", ["*"] * 6 + ["int", "int", "float"] + ["*"] * 3 + ["ltrx_stream_t"])
    assert _lib.PROTOTYPES["ltrx_norm_head_wgrad"] == ("int", ["*"] * 6 + ["int", "int"] + ["*"] * 3 + ["ltrx_stream_t"])
    assert _lib.PROTOTYPES["ltrx_norm_head_bwd_workspace_bytes"] == ("size_t", ["int", "int"])


def test_workspace_is_the_layernorm_backward_s(lib):
    for D in (256, 512, 768, 1024):
        for rows in (1, 37, 16383, 16384, 61440):
            # the fused backward takes over that kernel's grid and partial rows [da | db]
            assert lib.ltrx_norm_head_bwd_workspace_bytes(rows, D) == lib.ltrx_layernorm_bwd_workspace_bytes(rows, D) > 0
    assert lib.ltrx_norm_head_bwd_workspace_bytes(0, 512) == 0 and lib.ltrx_norm_head_bwd_workspace_bytes(64, 0) == 0


def test_refusals_happen_on_the_host(lib):
    p, odd = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004)
    pr = ctypes.c_int(-7)

    def fwd(D, x=p, w=p, y=None, rows=8):
        return lib.ltrx_norm_head_fwd(x, p, p, w, p, rows, D, 1e-6, p, p, p, y, None)

    def bwd(D, x=p, w=p, rows=8, out=ctypes.byref(pr)):
        return lib.ltrx_norm_head_bwd_partial(p, x, p, w, p, p, rows, D, 1e-6, p, p, out, None)

    def wgrad(D, x=p, a=p, rows=8, dw=p):
        return lib.ltrx_norm_head_wgrad(p, x, a, p, p, p, rows, D, dw, p, p, None)

    for D in (144, 96, 1280, 2048):
        assert fwd(D) == -2 and bwd(D) == -2 and wgrad(D) == -2, D
    assert fwd(512, x=odd) == -2 and fwd(512, w=odd) == -2 and fwd(512, y=odd) == -2
    assert bwd(512, x=odd) == -2 and bwd(512, w=odd) == -2
    assert fwd(512, x=None) == -1 and fwd(512, rows=0) == -1 and fwd(1) == -1
    assert bwd(512, x=None) == -1 and bwd(512, rows=0) == -1 and bwd(512, out=None) == -1
    assert wgrad(512, x=odd) == -2 and wgrad(512, a=odd) == -2
    assert wgrad(512, x=None) == -1 and wgrad(512, rows=0) == -1 and wgrad(512, dw=None) == -1
    assert pr.value == -7
