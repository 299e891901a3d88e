"""The Python side of the libltrx calls, no GPU.

  * Marshalling: every launcher of allrank_amd/kernels.py is called with CPU tensors and a recording stand-in for the library; the
    recorded argument list must equal an expectation written by header parameter NAME (the names are parsed from include/ltrx.h here),
    every parameter named.  The inputs are chosen so that a value in the wrong slot shows: operands are column slices of wider buffers
    (row stride != column count), the row count is smaller than the buffers', and no two integer arguments of a call are equal.
  * Arity: every ``<something>.ltrx_*(...)`` call in allrank_amd/**/*.py passes as many positional arguments as the header declares
    parameters (at least as many where it passes a star-argument) -- ctypes would say so only when the line runs on a GPU.
"""
import ast
import ctypes
import glob
import os
import re

import pytest
import torch

from allrank_amd import _lib, kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_names():
    """{entry point: [parameter names]} of include/ltrx.h"""
    with open(_lib.HEADER_PATH) as fh:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", fh.read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(ltrx_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [] if m.group(2).strip() in ("", "void") else m.group(2).split(",")
        out[m.group(1)] = [re.search(r"(\w+)\s*$", q).group(1) for q in params]
    return out


NAMES = _header_names()
ST = ctypes.c_void_p(0x5EED)                                  # the stream argument: handed through as it is


class Recorder(object):
    """stands in for the bound library: records ``(name, [arguments])``, returns 0 -- or ``returns[name]``, a query's byte count --
    and writes ``rows_out`` through a by-reference argument"""

    def __init__(self, returns=None, rows_out=0):
        self.calls, self.returns, self.rows_out = [], returns or {}, rows_out

    def __getattr__(self, name):
        def call(*args):
            plain = []
            for a in args:
                if hasattr(a, "_obj"):                        # ctypes.byref(c_int)
                    a._obj.value = self.rows_out
                    a = "byref"
                elif isinstance(a, ctypes.c_void_p):
                    a = a.value
                plain.append(a)
            self.calls.append((name, plain))
            return self.returns.get(name, 0)
        return call


def _expect(rec, name, same=(), **by_name):
    """the ONE recorded call is ``name`` with exactly the header's parameters, each holding ``by_name[parameter]``; apart from the
    parameters listed together in ``same`` (equal by the kernel's contract), no two integer arguments are equal"""
    assert [c[0] for c in rec.calls] == [name], rec.calls
    args = rec.calls[0][1]
    assert set(by_name) == set(NAMES[name]) and len(NAMES[name]) == len(_lib.SIGNATURES[name][1]) == len(args), (name, len(args))
    for pname, got in zip(NAMES[name], args):
        want = by_name[pname]
        assert got == want and type(got) is type(want), (name, pname, got, want)
    ints = {}
    for pname, got in zip(NAMES[name], args):
        if isinstance(got, int):
            assert got not in ints or {pname, ints[got]} <= set(same), (name, pname, ints[got], got)
            ints[got] = pname


def f32(*shape):
    return torch.arange(int(torch.tensor(shape).prod()), dtype=torch.float32).reshape(shape)


def u8(n):
    return torch.zeros(n, dtype=torch.uint8)


def i32(n):
    return torch.zeros(n, dtype=torch.int32)


def test_header_names_cover_the_binding_table():
    assert set(NAMES) == set(_lib.SIGNATURES)
    assert all(len(NAMES[n]) == len(_lib.SIGNATURES[n][1]) for n in NAMES)
    assert NAMES["ltrx_gemm_nt"][:5] == ["A", "lda", "B", "ldb", "B_image"] and NAMES["ltrx_gemm_nt"][-1] == "stream"


@pytest.mark.parametrize("aux_kind", ["none", "matrix", "bits"])
def test_gemm_nt(aux_kind):
    a, b, out = f32(9, 24)[:, :12], f32(20, 16)[:, :12], f32(9, 28)[:, :20]          # M 7 of 9 rows, N 20, K 12; strides 24, 16, 28
    bias, step = f32(20), i32(1)
    aux, act, ldaux = {"none": (None, 1, 0), "matrix": (f32(9, 36)[:, :20], 3, 36), "bits": (u8(64), 5, 0)}[aux_kind]
    rec = Recorder()
    K.gemm_nt(rec, ST, a, b, out, 7, bias, act, aux, 0.25, 4242, step, 2, 8, ctypes.c_void_p(0xABC0), "w")
    _expect(rec, "ltrx_gemm_nt", A=a.data_ptr(), lda=24, B=b.data_ptr(), ldb=16, B_image=0xABC0, C=out.data_ptr(), ldc=28, M=7, N=20, K=12,
            bias=bias.data_ptr(), act=act, aux=None if aux is None else aux.data_ptr(), ldaux=ldaux, drop_p=0.25, drop_seed=4242,
            drop_step=step.data_ptr(), strict=2, tile=8, stream=ST.value)


def test_gemm_nt_defaults_are_the_plain_product():
    a, b, out = f32(9, 24)[:, :12], f32(20, 16)[:, :12], f32(9, 28)[:, :20]
    rec = Recorder()
    K.gemm_nt(rec, ST, a, b, out, 7)
    _expect(rec, "ltrx_gemm_nt", same=("act", "ldaux", "drop_seed", "strict", "tile"),
            A=a.data_ptr(), lda=24, B=b.data_ptr(), ldb=16, B_image=None, C=out.data_ptr(), ldc=28, M=7, N=20, K=12, bias=None, act=0,
            aux=None, ldaux=0, drop_p=0.0, drop_seed=0, drop_step=None, strict=0, tile=0, stream=ST.value)


def test_gemm_tn_and_its_workspace():
    dy, x = f32(9, 24)[:, :20], f32(9, 16)[:, :12]                                    # the contiguous form has lda == NP; this one not
    gw, gb, ws = f32(20, 12), f32(20), u8(64)
    rec = Recorder()
    K.gemm_tn(rec, ST, dy, x, gw, gb, 7, 2, 9, ws, "w")
    _expect(rec, "ltrx_gemm_tn", A=dy.data_ptr(), lda=24, B=x.data_ptr(), ldb=16, C=gw.data_ptr(), bias_out=gb.data_ptr(), M=7, NP=20, KP=12,
            strict=2, tile=9, ws=ws.data_ptr(), stream=ST.value)
    dense = f32(9, 20)
    rec = Recorder()
    K.gemm_tn(rec, ST, dense, x, gw, None, 7, 2, 9, ws)
    _expect(rec, "ltrx_gemm_tn", same=("lda", "NP"), A=dense.data_ptr(), lda=20, B=x.data_ptr(), ldb=16, C=gw.data_ptr(), bias_out=None, M=7,
            NP=20, KP=12, strict=2, tile=9, ws=ws.data_ptr(), stream=ST.value)
    rec = Recorder(returns={"ltrx_gemm_tn_workspace_bytes": 1000})
    got = K.gemm_tn_workspace(rec, 7, 20, 12, x)
    _expect(rec, "ltrx_gemm_tn_workspace_bytes", M=7, NP=20, KP=12)
    assert got.dtype == torch.uint8 and got.numel() == 1000
    assert K.gemm_tn_workspace(Recorder(), 7, 20, 12, x).numel() == 64               # never an empty buffer


def _qkv(form, rows, d, stride):
    if form == "packed":                                      # column views of one [rows, 3d] projection
        qkv = f32(rows, 3 * d)
        return qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], 3 * d
    return tuple(f32(rows, stride)[:, :d] for _ in range(3)) + (stride,)


@pytest.mark.parametrize("form", ["packed", "separate"])
def test_mha_fwd_and_bwd(form):
    B, L, h, dk = 2, 5, 3, 8
    d = h * dk
    q, k, v, rs = _qkv(form, B * L, d, 40)
    dq, dk_, dv, drs = _qkv(form, B * L, d, 52)
    if form == "packed":                                      # the gradient buffer: another stride than the projection's
        wide = f32(B * L, 3 * d + 4)
        dq, dk_, dv, drs = wide[:, :d], wide[:, d:2 * d], wide[:, 2 * d:3 * d], 3 * d + 4
        assert (k.data_ptr(), v.data_ptr()) == (q.data_ptr() + 4 * d, q.data_ptr() + 8 * d)
    o, do, lse = f32(B * L, 28)[:, :d], f32(B * L, d), f32(B, h, L)
    kpm, step, cu, order, ws = u8(B * L), i32(1), i32(B + 1), i32(B), u8(64)
    rec = Recorder()
    K.mha_fwd(rec, ST, q, k, v, kpm, B, L, h, o, lse, 0.125, 99991, step, cu, order, 1)
    _expect(rec, "ltrx_mha_fwd", q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), key_pad_mask=kpm.data_ptr(), B=B, L=L, h=h, d_k=dk,
            row_stride=rs, o=o.data_ptr(), o_row_stride=28, lse_out=lse.data_ptr(), p_drop=0.125, seed=99991, seed_step=step.data_ptr(),
            cu_seqlens=cu.data_ptr(), slate_order=order.data_ptr(), mode=1, stream=ST.value)
    rec = Recorder()
    K.mha_bwd(rec, ST, q, k, v, None, o, do, lse, B, L, h, dq, dk_, dv, 0.125, 99991, None, None, None, 1, ws)
    _expect(rec, "ltrx_mha_bwd", q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), key_pad_mask=None, o=o.data_ptr(), dout=do.data_ptr(),
            lse=lse.data_ptr(), B=B, L=L, h=h, d_k=dk, row_stride=rs, o_row_stride=28, dq=dq.data_ptr(), dk=dk_.data_ptr(),
            dv=dv.data_ptr(), d_row_stride=drs, p_drop=0.125, seed=99991, seed_step=None, cu_seqlens=None, slate_order=None, mode=1,
            ws=ws.data_ptr(), stream=ST.value)
    # [B, L, d] operands (the autograd bindings' form): the row stride is the items', not the slates'
    q3, o3 = f32(B, L, 40)[:, :, :d], f32(B, L, d)
    rec = Recorder()
    K.mha_fwd(rec, ST, q3, q3, q3, kpm, B, L, h, o3, lse, 0.0, 7, None, None, None, 0)
    assert rec.calls[0][1][8] == 40 and rec.calls[0][1][10] == d and NAMES["ltrx_mha_fwd"][8] == "row_stride"
    rec = Recorder(returns={"ltrx_mha_bwd_workspace_bytes": 4096})
    assert K.mha_bwd_workspace(rec, B, L, h, dk, 1, q).numel() == 4096
    _expect(rec, "ltrx_mha_bwd_workspace_bytes", B=B, L=L, h=h, d_k=dk, mode=1)


def test_layernorm_calls():
    x, res, a, b = f32(9, 12), f32(9, 12), f32(12), f32(12)
    xsum, y, mean, rstd, step, ws = f32(9, 12), f32(9, 12), f32(9), f32(9), i32(1), u8(64)
    rec = Recorder()
    K.layernorm_fwd(rec, ST, x, res, a, b, 7, 1e-6, xsum, y, mean, rstd, 0.5, 31337, step)
    _expect(rec, "ltrx_layernorm_fwd", x=x.data_ptr(), res=res.data_ptr(), a=a.data_ptr(), b=b.data_ptr(), rows=7, D=12, eps=1e-6,
            xsum_out=xsum.data_ptr(), y_out=y.data_ptr(), mean_out=mean.data_ptr(), rstd_out=rstd.data_ptr(), res_drop_p=0.5,
            drop_seed=31337, drop_step=step.data_ptr(), stream=ST.value)
    rec = Recorder()
    K.layernorm_fwd(rec, ST, x, None, a, b, 7, 1e-6, None, y, mean, rstd)
    _expect(rec, "ltrx_layernorm_fwd", x=x.data_ptr(), res=None, a=a.data_ptr(), b=b.data_ptr(), rows=7, D=12, eps=1e-6, xsum_out=None,
            y_out=y.data_ptr(), mean_out=mean.data_ptr(), rstd_out=rstd.data_ptr(), res_drop_p=0.0, drop_seed=0, drop_step=None,
            stream=ST.value)
    dy, dres, dx, da, db = f32(9, 12), f32(9, 12), f32(9, 12), f32(12), f32(12)
    rec = Recorder()
    K.layernorm_bwd(rec, ST, dy, xsum, a, mean, rstd, dres, 7, 1e-6, dx, da, db, ws)
    _expect(rec, "ltrx_layernorm_bwd", dy=dy.data_ptr(), xsum=xsum.data_ptr(), a=a.data_ptr(), mean=mean.data_ptr(), rstd=rstd.data_ptr(),
            dres_in=dres.data_ptr(), rows=7, D=12, eps=1e-6, dx_out=dx.data_ptr(), da_out=da.data_ptr(), db_out=db.data_ptr(),
            ws=ws.data_ptr(), stream=ST.value)
    rec = Recorder(rows_out=5)
    assert K.layernorm_bwd_partial(rec, ST, dy, xsum, a, mean, rstd, None, 7, 1e-6, dx, ws) == 5
    _expect(rec, "ltrx_layernorm_bwd_partial", dy=dy.data_ptr(), xsum=xsum.data_ptr(), a=a.data_ptr(), mean=mean.data_ptr(),
            rstd=rstd.data_ptr(), dres_in=None, rows=7, D=12, eps=1e-6, dx_out=dx.data_ptr(), ws=ws.data_ptr(), partial_rows_out="byref",
            stream=ST.value)
    rec = Recorder(returns={"ltrx_layernorm_bwd_workspace_bytes": 777})
    assert K.layernorm_bwd_workspace(rec, 7, 12, x).numel() == 777
    _expect(rec, "ltrx_layernorm_bwd_workspace_bytes", rows=7, D=12)


def test_score_head_and_activation_calls():
    x, w, b, sc = f32(9, 12), f32(12), f32(1), f32(9)
    ds, dx, dw, db, ws = f32(9), f32(9, 12), f32(12), f32(1), u8(64)
    rec = Recorder()
    K.score_head_fwd(rec, ST, x, w, b, 7, sc)
    _expect(rec, "ltrx_score_head_fwd", x=x.data_ptr(), w=w.data_ptr(), b=b.data_ptr(), M=7, D=12, scores=sc.data_ptr(), stream=ST.value)
    rec = Recorder()
    K.score_head_bwd(rec, ST, ds, x, w, 7, dx, dw, db, ws)
    _expect(rec, "ltrx_score_head_bwd", dscores=ds.data_ptr(), x=x.data_ptr(), w=w.data_ptr(), M=7, D=12, dx=dx.data_ptr(), dw=dw.data_ptr(),
            db=db.data_ptr(), ws=ws.data_ptr(), stream=ST.value)
    rec = Recorder(returns={"ltrx_score_head_bwd_workspace_bytes": 320})
    assert K.score_head_bwd_workspace(rec, 7, 12, x).numel() == 320
    _expect(rec, "ltrx_score_head_bwd_workspace_bytes", M=7, D=12)
    rec = Recorder()
    K.out_act_fwd(rec, ST, sc, 7, 2, dx)
    _expect(rec, "ltrx_out_act_fwd", z=sc.data_ptr(), n=7, kind=2, y=dx.data_ptr(), stream=ST.value)
    rec = Recorder()
    K.out_act_bwd(rec, ST, ds, sc, 7, 2, dx)
    _expect(rec, "ltrx_out_act_bwd", dy=ds.data_ptr(), y=sc.data_ptr(), n=7, kind=2, dz=dx.data_ptr(), stream=ST.value)


def test_split_image_and_gather_rows_cu():
    src, dst = f32(40), f32(40)
    rec = Recorder()
    K.split_image(rec, ST, src, dst)
    _expect(rec, "ltrx_split_image", src=src.data_ptr(), dst=dst.data_ptr(), n=40, stream=ST.value)
    B, L = 3, 5
    # the source is the dense grid (ld_src is its column count by contract); the packed rows land in a padded buffer: stride 24
    xb, cu, rows_buf, idx = f32(2, L, 12), i32(B + 1), f32(32, 24)[:, :12], i32(32)
    rec = Recorder()
    K.gather_rows_cu(rec, ST, xb, cu, B, L, 12, 32, rows_buf, idx)
    _expect(rec, "ltrx_gather_rows_cu", same=("ld_src", "cols"), src=xb.data_ptr(), ld_src=12, cu_seqlens=cu.data_ptr(), B=B, L=L, cols=12,
            rows=32, dst=rows_buf.data_ptr(), ld_dst=24, idx_out=idx.data_ptr(), stream=ST.value)
    ib, ranks = torch.zeros((2, L), dtype=torch.int64), torch.zeros(32, dtype=torch.int64)             # int64: pairs of 32-bit words
    rec = Recorder()
    K.gather_rows_cu(rec, ST, ib, cu, B, L, 2, 32, ranks)
    _expect(rec, "ltrx_gather_rows_cu", same=("ld_src", "cols", "ld_dst"), src=ib.data_ptr(), ld_src=2, cu_seqlens=cu.data_ptr(), B=B, L=L,
            cols=2, rows=32, dst=ranks.data_ptr(), ld_dst=2, idx_out=None, stream=ST.value)
    y, y_c = f32(B, L), f32(32)                                                                          # labels: one column
    rec = Recorder()
    K.gather_rows_cu(rec, ST, y, cu, B, L, 1, 32, y_c)
    _expect(rec, "ltrx_gather_rows_cu", same=("ld_src", "cols", "ld_dst"), src=y.data_ptr(), ld_src=1, cu_seqlens=cu.data_ptr(), B=B, L=L,
            cols=1, rows=32, dst=y_c.data_ptr(), ld_dst=1, idx_out=None, stream=ST.value)


def i64(n):
    return torch.zeros(n, dtype=torch.int64)


@pytest.mark.parametrize("with_x", [True, False])
def test_ingest_batch(with_x):
    B, L, F = 3, 5, 12
    x, y = (f32(B, L, F) if with_x else None), f32(B, L)
    x_dst, y_dst, mask = f32(B * L, 16)[:, :F], f32(B, L), u8(B * L)                  # padded operand rows: stride 16
    rec = Recorder()
    K.ingest_batch(rec, ST, x, y, -1, x_dst, y_dst, mask)
    # the packed layouts' form (x None, nx 0): F and ld_dst still state the row shape, the destination is NULL
    _expect(rec, "ltrx_ingest_batch", x=x.data_ptr() if with_x else None, y=y.data_ptr(), nx=B * L * F if with_x else 0, ny=B * L, F=F,
            ld_dst=16, pad_value=-1.0, x_dst=x_dst.data_ptr() if with_x else None, y_dst=y_dst.data_ptr(), mask_dst=mask.data_ptr(),
            stream=ST.value)


def test_index_layout_movers():
    B, L, F = 3, 5, 12
    cu, idx = i32(B + 1), i32(32)
    rec = Recorder()
    K.packed_row_index(rec, ST, cu, B, L, 11, idx)
    _expect(rec, "ltrx_packed_row_index", cu_seqlens=cu.data_ptr(), B=B, L=L, n=11, idx=idx.data_ptr(), stream=ST.value)
    # features: rows of a wider source (stride 20) into the padded operand rows (stride 16); n 11 valid rows, 32 rows written
    src, dst = f32(B * L, 20)[:, :F], f32(32, 16)[:, :F]
    rec = Recorder()
    K.gather_rows(rec, ST, src, idx, 11, 32, F, dst, "w")
    _expect(rec, "ltrx_gather_rows", src=src.data_ptr(), ld_src=20, idx=idx.data_ptr(), n=11, n_pad=32, cols=F, dst=dst.data_ptr(),
            ld_dst=16, stream=ST.value)
    # d loss / d scores: the [B, L] grid of one column into a vector -- and of 4 output units into [rows, 4]
    g1, v1 = f32(B, L), f32(32)
    rec = Recorder()
    K.gather_rows(rec, ST, g1, idx, 11, 32, 1, v1)
    _expect(rec, "ltrx_gather_rows", same=("ld_src", "cols", "ld_dst"), src=g1.data_ptr(), ld_src=1, idx=idx.data_ptr(), n=11, n_pad=32,
            cols=1, dst=v1.data_ptr(), ld_dst=1, stream=ST.value)
    g4, v4 = f32(B, L, 4), f32(32, 6)[:, :4]
    rec = Recorder()
    K.gather_rows(rec, ST, g4, idx, 11, 32, 4, v4)
    _expect(rec, "ltrx_gather_rows", same=("ld_src", "cols"), src=g4.data_ptr(), ld_src=4, idx=idx.data_ptr(), n=11, n_pad=32, cols=4,
            dst=v4.data_ptr(), ld_dst=6, stream=ST.value)
    rec = Recorder()
    K.scatter_rows(rec, ST, v4, idx, 11, 4, g4)
    _expect(rec, "ltrx_scatter_rows", same=("cols", "ld_dst"), src=v4.data_ptr(), ld_src=6, idx=idx.data_ptr(), n=11, cols=4,
            dst=g4.data_ptr(), ld_dst=4, stream=ST.value)
    rec = Recorder()
    K.scatter_rows(rec, ST, v1, idx, 11, 1, g1)
    _expect(rec, "ltrx_scatter_rows", same=("ld_src", "cols", "ld_dst"), src=v1.data_ptr(), ld_src=1, idx=idx.data_ptr(), n=11, cols=1,
            dst=g1.data_ptr(), ld_dst=1, stream=ST.value)


def test_cu_layout_movers():
    B, L = 3, 5
    cu = i32(B + 1)
    sc, grid = f32(32, 6)[:, :4], f32(B, L, 4)                                        # packed rows of stride 6 -> the dense grid
    rec = Recorder()
    K.scatter_rows_cu(rec, ST, sc, cu, B, L, 4, 32, grid)
    _expect(rec, "ltrx_scatter_rows_cu", same=("cols", "ld_dst"), src=sc.data_ptr(), ld_src=6, cu_seqlens=cu.data_ptr(), B=B, L=L, cols=4,
            rows=32, dst=grid.data_ptr(), ld_dst=4, stream=ST.value)
    s1, g1 = f32(32), f32(B, L)
    rec = Recorder()
    K.scatter_rows_cu(rec, ST, s1, cu, B, L, 1, 32, g1)
    _expect(rec, "ltrx_scatter_rows_cu", same=("ld_src", "cols", "ld_dst"), src=s1.data_ptr(), ld_src=1, cu_seqlens=cu.data_ptr(), B=B, L=L,
            cols=1, rows=32, dst=g1.data_ptr(), ld_dst=1, stream=ST.value)
    buf = f32(40, 24)[:, :12]                                                          # 32 of the buffer's 40 rows
    rec = Recorder()
    K.zero_rows_cu(rec, ST, buf, cu, B, 32)
    _expect(rec, "ltrx_zero_rows_cu", x=buf.data_ptr(), ld=24, cols=12, cu_seqlens=cu.data_ptr(), B=B, rows=32, stream=ST.value)


@pytest.mark.parametrize("with_pos", [True, False])
def test_assemble_packed(with_pos):
    B, L, F = 3, 5, 12
    x_items, y_items, offsets, slates, cu = f32(40, F), f32(40), i64(9), i64(B), i32(B + 1)
    x_out, y_out, idx, pos = f32(32, 16)[:, :F], f32(B, L), i32(32), (i64(32) if with_pos else None)
    rec = Recorder()
    K.assemble_packed(rec, ST, x_items, y_items, offsets, slates, cu, B, L, 32, x_out, y_out, idx, pos)
    _expect(rec, "ltrx_assemble_packed", x_items=x_items.data_ptr(), y_items=y_items.data_ptr(), offsets=offsets.data_ptr(),
            slates=slates.data_ptr(), cu_seqlens=cu.data_ptr(), B=B, L=L, F=F, rows=32, x_out=x_out.data_ptr(), ld_x=16,
            y_out=y_out.data_ptr(), idx_out=idx.data_ptr(), pos_out=pos.data_ptr() if with_pos else None, stream=ST.value)


def test_a_failed_call_raises_with_its_label():
    a, b, out = f32(9, 12), f32(20, 12), f32(9, 20)
    with pytest.raises(RuntimeError, match=r"gemm_nt\(fwd\) failed: unsupported shape"):
        K.gemm_nt(Recorder(returns={"ltrx_gemm_nt": -2}), ST, a, b, out, 7, what="gemm_nt(fwd)")


# ------------------------------------------------------------------------------------------------------------------
# arity of every ltrx_* call the package writes out
# ------------------------------------------------------------------------------------------------------------------
def _ltrx_calls():
    for path in sorted(glob.glob(os.path.join(ROOT, "allrank_amd", "**", "*.py"), recursive=True)):
        with open(path) as fh:
            tree = ast.parse(fh.read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in _lib.SIGNATURES:
                yield os.path.relpath(path, ROOT), node


def test_every_ltrx_call_passes_the_headers_argument_count():
    seen = set()
    for path, node in _ltrx_calls():
        name, want = node.func.attr, len(_lib.SIGNATURES[node.func.attr][1])
        assert not node.keywords, (path, node.lineno, name, "ctypes takes positional arguments only")
        starred = [a for a in node.args if isinstance(a, ast.Starred)]
        plain = len(node.args) - len(starred)
        assert (plain <= want) if starred else (plain == want), (path, node.lineno, name, plain, want)
        seen.add(name)
    # the scan sees the launchers' calls, the single-site calls the engine keeps and the loss launchers
    assert {"ltrx_gemm_nt", "ltrx_mha_bwd", "ltrx_norm_head_fwd", "ltrx_weight_images", "ltrx_fc_listnet_step", "ltrx_listnet_fwd_bwd",
            "ltrx_adam_step"} <= seen and len(seen) >= 60, sorted(seen)


def test_each_launched_call_is_written_once():
    """the launches kernels.py states appear nowhere else in the package (a byte-count query may: the engine sizes one workspace for
    the largest of several shapes)"""
    mine = {node.func.attr for path, node in _ltrx_calls()
            if path == os.path.join("allrank_amd", "kernels.py") and not node.func.attr.endswith("_workspace_bytes")}
    assert mine == {"ltrx_gemm_nt", "ltrx_gemm_tn", "ltrx_mha_fwd", "ltrx_mha_bwd", "ltrx_layernorm_fwd", "ltrx_layernorm_bwd",
                    "ltrx_layernorm_bwd_partial", "ltrx_score_head_fwd", "ltrx_score_head_bwd", "ltrx_out_act_fwd", "ltrx_out_act_bwd",
                    "ltrx_split_image", "ltrx_gather_rows_cu",
                    # the packing calls
                    "ltrx_gather_rows", "ltrx_scatter_rows", "ltrx_packed_row_index", "ltrx_scatter_rows_cu", "ltrx_zero_rows_cu",
                    "ltrx_assemble_packed", "ltrx_ingest_batch"}, sorted(mine)
    count = {}
    for path, node in _ltrx_calls():
        if node.func.attr in mine:
            count[node.func.attr] = count.get(node.func.attr, 0) + 1
    assert set(count.values()) == {1}, {k: v for k, v in count.items() if v != 1}
