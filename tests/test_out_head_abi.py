"""CPU-side checks of ltrx_out_head_fwd and ltrx_rank_slates_rows_cu: declared in include/ltrx.h, bound from it, exported by the built
library, refusing bad arguments before any HIP call (no kernel is launched), and marshalled by their launchers
(allrank_amd/outhead.py, handed on by allrank_amd/kernels.py) by header parameter name, with the recorder of
tests/test_kernel_calls_cpu.py."""
import ctypes
import types

import pytest

from tests.test_kernel_calls_cpu import Recorder, _expect, ST, f32, i32, i64

FAKE = ctypes.c_void_p(4096)                           # 16-byte aligned, never dereferenced: the argument checks come first


@pytest.fixture(scope="module")
def lib():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _head(lib, x=FAKE, ldx=144, W=FAKE, bias=FAKE, rows=5, D=144, n_out=4, act=1, out=FAKE, score=FAKE):
    return lib.ltrx_out_head_fwd(x, ldx, W, bias, rows, D, n_out, act, out, score, None)


def _rank(lib, out=FAKE, n_out=4, cu=FAKE, B=2, max_len=8, F=4, L=8, x_out=FAKE, y_out=FAKE, x=FAKE, y=FAKE, ids=None):
    return lib.ltrx_rank_slates_rows_cu(out, n_out, x, y, None, None, None, ids, cu, None, B, max_len, F, L, None, x_out, y_out, None)


@pytest.mark.parametrize("name", ["ltrx_out_head_fwd", "ltrx_rank_slates_rows_cu"])
def test_the_prototypes_are_declared_bound_and_exported(lib, name):
    from allrank_amd import _lib
    assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and hasattr(lib, name)
    assert _lib.SIGNATURES[name][0] is ctypes.c_int and _lib.PROTOTYPES[name][1][-1] == "ltrx_stream_t"
    assert lib.ltrx_version() == 130


def test_out_head_refuses_before_any_hip_call(lib):
    for bad in (dict(x=None), dict(W=None), dict(bias=None), dict(out=None, score=None), dict(rows=0), dict(D=0), dict(n_out=0),
                dict(ldx=140), dict(act=3), dict(act=-1)):
        assert _head(lib, **bad) == -1, bad
    for unsupported in (dict(n_out=9), dict(D=6, ldx=8), dict(D=1028, ldx=1028), dict(ldx=146), dict(x=ctypes.c_void_p(4100))):
        assert _head(lib, **unsupported) == -2, unsupported


def test_rank_rows_refuses_as_rank_slates_cu_does(lib):
    from allrank_amd import _lib
    for bad in (dict(out=None), dict(n_out=0), dict(cu=None), dict(x_out=None), dict(y_out=None), dict(B=0), dict(F=0), dict(max_len=9),
                dict(max_len=0), dict(y=None), dict(x=None, y=None), dict(ids=FAKE)):
        assert _rank(lib, **bad) == -1, bad
    over = _lib.MAX_METRIC_SLATE_LEN + 1
    assert _rank(lib, max_len=over, L=over) == -2


def test_the_launchers_pass_every_header_parameter():
    from allrank_amd import kernels as K, outhead
    assert K.out_head_fwd is outhead.out_head_fwd and K.rank_slates_rows_cu is outhead.rank_slates_rows_cu
    x, w, b, out, score = f32(9, 16)[:, :12], f32(3, 12), f32(3), f32(9, 3), f32(9)          # rows of stride 16, 7 of them
    rec = Recorder()
    assert K.out_head_fwd(rec, ST, x, w, b, 7, 2, out, score) is True
    _expect(rec, "ltrx_out_head_fwd", x=x.data_ptr(), ldx=16, W=w.data_ptr(), bias=b.data_ptr(), rows=7, D=12, n_out=3, act=2,
            out=out.data_ptr(), score=score.data_ptr(), stream=ST.value)
    assert K.out_head_fwd(Recorder(returns={"ltrx_out_head_fwd": -2}), ST, x, w, b, 7, 2, out) is False      # the caller's GEMM sequence
    with pytest.raises(RuntimeError, match="out_head_fwd failed: invalid argument"):
        K.out_head_fwd(Recorder(returns={"ltrx_out_head_fwd": -1}), ST, x, w, b, 7, 2, out)
    B, L, F, ml = 3, 7, 12, 5
    rows, cu, order, perm, x_out, y_out = f32(11, 4), i32(B + 1), i32(B), i32(11), f32(B, L, F), f32(B, L)
    slates, ids = types.SimpleNamespace(x_items=f32(40, F), y_items=f32(40), offsets=i64(9)), i64(B)
    rec = Recorder()
    K.rank_slates_rows_cu(rec, ST, rows, cu, order, B, ml, L, x_out, y_out, perm, slates=slates, ids=ids)
    _expect(rec, "ltrx_rank_slates_rows_cu", out=rows.data_ptr(), n_out=4, x=None, y=None, x_items=slates.x_items.data_ptr(),
            y_items=slates.y_items.data_ptr(), offsets=slates.offsets.data_ptr(), ids=ids.data_ptr(), cu_seqlens=cu.data_ptr(),
            slate_order=order.data_ptr(), B=B, max_len=ml, F=F, L=L, perm=perm.data_ptr(), x_out=x_out.data_ptr(), y_out=y_out.data_ptr(),
            stream=ST.value)
