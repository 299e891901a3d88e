"""The Python side of the libltrx calls, no GPU.

  * Marshalling: every launcher of allrank_amd/kernels.py -- the scoring model's calls, the packing calls, the training step's own
    calls, ranking, clicks and the MFMA self-test -- is called with CPU tensors and a recording stand-in for the library; the
    recorded argument list must equal an expectation written by header parameter NAME (the names are parsed from include/ltrx.h here),
    every parameter named.  The inputs are chosen so that a value in the wrong slot shows: operands are column slices of wider buffers
    (row stride != column count), the row count is smaller than the buffers', and no two integer arguments of a call are equal.
  * Arity: every ``<something>.ltrx_*(...)`` call in allrank_amd/**/*.py passes as many positional arguments as the header declares
    parameters (at least as many where it passes a star-argument) -- ctypes would say so only when the line runs on a GPU.
  * One statement per launch: a launch kernels.py states is written nowhere else, the modules that launch through it state none of
    their own, and every launch it states has a marshalling test here.
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
    """stands in for the bound library: records ``(name, [arguments])`` and returns 0 -- or ``returns[name]``, a query's result.  A
    by-reference argument is recorded as "byref" and receives ``outs[its parameter name]`` (default ``rows_out``); a ctypes array is
    recorded as the list of its values -- or, named in ``outs``, filled with those values and recorded as "out"; a pointer named in
    ``reads`` is recorded as the value of that ctypes type found at its address WHILE the call runs"""

    def __init__(self, returns=None, rows_out=0, outs=None, reads=None):
        self.calls, self.returns, self.rows_out, self.outs, self.reads = [], returns or {}, rows_out, outs or {}, reads or {}

    def __getattr__(self, name):
        def call(*args):
            plain = []
            for pname, a in zip(NAMES.get(name, []) + [None] * len(args), args):
                if hasattr(a, "_obj"):                        # ctypes.byref(c_int)
                    a._obj.value = self.outs.get(pname, self.rows_out)
                    a = "byref"
                elif isinstance(a, ctypes.Array):
                    if pname in self.outs:
                        a[:] = self.outs[pname]
                        a = "out"
                    else:
                        a = list(a)
                elif isinstance(a, ctypes.c_void_p):
                    a = self.reads[pname].from_address(a.value).value if pname in self.reads else a.value
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


# ------------------------------------------------------------------------------------------------------------------
# the training step's own calls
# ------------------------------------------------------------------------------------------------------------------
def test_step_plumbing_calls():
    src, dst, step, word = f32(9, 12), f32(9, 12), i32(1), i32(1)
    rec = Recorder()
    K.bump_u32(rec, ST, word)
    _expect(rec, "ltrx_bump_u32", word=word.data_ptr(), stream=ST.value)
    rec = Recorder()
    K.dropout_apply(rec, ST, src, 7, 0.25, 4242, step, dst)                           # 7 of 9 rows: n = 7 * 12
    _expect(rec, "ltrx_dropout_apply", src=src.data_ptr(), dst=dst.data_ptr(), n=84, p=0.25, seed=4242, drop_step=step.data_ptr(),
            stream=ST.value)
    a, out, ws = f32(9, 24)[:, :20], f32(20), u8(64)
    rec = Recorder()
    K.colsum(rec, ST, a, 7, out, ws)
    _expect(rec, "ltrx_colsum", a=a.data_ptr(), M=7, N=20, ld=24, out=out.data_ptr(), accumulate=0, ws=ws.data_ptr(), stream=ST.value)
    rec = Recorder(returns={"ltrx_colsum_workspace_bytes": 512})
    assert K.colsum_workspace(rec, 7, 20, a).numel() == 512
    _expect(rec, "ltrx_colsum_workspace_bytes", M=7, N=20)
    rec = Recorder()
    K.relu_bwd(rec, ST, dst, src, 7, 1.25)
    _expect(rec, "ltrx_relu_bwd", dr_inout=dst.data_ptr(), r_post_act=src.data_ptr(), n=84, scale=1.25, stream=ST.value)
    rec = Recorder()
    K.scale_inplace(rec, ST, src, 84, 3.5)
    _expect(rec, "ltrx_scale_inplace", x=src.data_ptr(), n=84, s=3.5, stream=ST.value)


@pytest.mark.parametrize("padded", [True, False])
def test_weight_images_and_transpose_batch(padded):
    src, src_i, dst, dst_i, desc, tstart = f32(40), f32(40), f32(24), f32(24), i64(12), i32(4)
    w0, w0_pad, w0_pad_i = f32(6, 10), f32(6, 32), f32(6, 32)                         # [6, 10] into rows of 32
    rec = Recorder()
    K.weight_images(rec, ST, src, src_i, dst, dst_i, desc, tstart, 3, 5, *((w0, w0_pad, w0_pad_i) if padded else ()))
    _expect(rec, "ltrx_weight_images", same=() if padded else ("pad_rows", "pad_cols", "pad_ld"),
            src_base=src.data_ptr(), nflat=40, src_image=src_i.data_ptr(), dst_base=dst.data_ptr(), dst_image=dst_i.data_ptr(),
            desc=desc.data_ptr(), tile_start=tstart.data_ptr(), n=3, total_tiles=5, pad_src=w0.data_ptr() if padded else None,
            pad_rows=6 if padded else 0, pad_cols=10 if padded else 0, pad_ld=32 if padded else 0,
            pad_dst=w0_pad.data_ptr() if padded else None, pad_dst_image=w0_pad_i.data_ptr() if padded else None, stream=ST.value)
    rec = Recorder()
    K.transpose_batch(rec, ST, src, dst, desc, tstart, 3, 5)
    _expect(rec, "ltrx_transpose_batch", src_base=src.data_ptr(), dst_base=dst.data_ptr(), desc=desc.data_ptr(),
            tile_start=tstart.data_ptr(), n=3, total_tiles=5, stream=ST.value)


def _tn_problems():
    """three weight-gradient problems of different shapes and strides: (dy, x, gw, gb), 7 of 9 rows"""
    shapes = [((24, 20), (16, 12)), ((36, 28), (20, 8)), ((40, 40), (44, 32))]        # (stride, columns) of dy and of x; dy 2 dense
    return [(f32(9, sa)[:, :n], f32(9, sb)[:, :k], f32(n, k), f32(n)) for (sa, n), (sb, k) in shapes]


def _tn_expected(probs):
    at = lambda i: [t[i].data_ptr() for t in probs]  # noqa: E731
    return dict(nprob=3, A=at(0), lda=[24, 36, 40], B=at(1), ldb=[16, 20, 44], C=at(2), bias_out=at(3), M=7, NP=[20, 28, 40],
                KP=[12, 8, 32], strict=2, ws_bytes=4096)


SLABS = dict(slabs_out=[0x1000, 0x2000, 0x3000], bias_slabs_out=[0x100, 0, 0x300], splits_out=5)


@pytest.mark.parametrize("defer", [False, True])
def test_gemm_tn_group(defer):
    probs, ws = _tn_problems(), u8(4096)
    rec = Recorder(outs=SLABS)
    got = K.gemm_tn_group(rec, ST, probs, 7, 2, ws, defer, "w")
    _expect(rec, "ltrx_gemm_tn_group", ws=ws.data_ptr(), slabs_out="out" if defer else None, bias_slabs_out="out" if defer else None,
            splits_out="byref" if defer else None, stream=ST.value, **_tn_expected(probs))
    # slab i belongs to problem i; a problem without a bias slab reads as None
    assert got == (([0x1000, 0x2000, 0x3000], [0x100, None, 0x300], 5) if defer else None)


@pytest.mark.parametrize("defer", [False, True])
def test_gemm_tn_group_ln(defer):
    probs, ws, ln_ws = _tn_problems(), u8(4096), u8(64)
    dy, xsum, a, mean, rstd, dres, dx = f32(9, 12), f32(9, 12), f32(12), f32(9), f32(9), f32(9, 12), f32(9, 12)
    rec = Recorder(outs=dict(SLABS, partial_rows_out=6, side_taken_out=11))
    got = K.gemm_tn_group_ln(rec, ST, probs, 7, 2, ws, dy, xsum, a, mean, rstd, dres, 1e-6, dx, ln_ws, defer, "w")
    _expect(rec, "ltrx_gemm_tn_group_ln", same=("M", "rows"), ws=ws.data_ptr(), slabs_out="out" if defer else None,
            bias_slabs_out="out" if defer else None, splits_out="byref" if defer else None, dy=dy.data_ptr(), xsum=xsum.data_ptr(),
            a=a.data_ptr(), mean=mean.data_ptr(), rstd=rstd.data_ptr(), dres_in=dres.data_ptr(), rows=7, D=12, eps=1e-6,
            dx_out=dx.data_ptr(), ln_ws=ln_ws.data_ptr(), partial_rows_out="byref", side_wgs=0, side_taken_out="byref", stream=ST.value,
            **_tn_expected(probs))
    assert got == ((([0x1000, 0x2000, 0x3000], [0x100, None, 0x300], 5) if defer else None), 6, 11)


def test_tn_group_plan_and_reduce_group():
    probs, ws = _tn_problems(), u8(4096)
    want = _tn_expected(probs)
    for took in (1, 0):
        rec = Recorder(returns={"ltrx_debug_tn_group_plan": took})
        assert K.tn_group_plan(rec, probs, 7, 2, ws) is bool(took)
        _expect(rec, "ltrx_debug_tn_group_plan", splits_out="byref", need_bytes_out="byref",
                **{k: want[k] for k in ("nprob", "M", "NP", "KP", "lda", "ldb", "strict", "ws_bytes")})
    entries = [(0x1000, 5, 240, 240, 0x9000), (0x2000, 4, 20, 20, 0x9100), (0x3000, 6, 24, 12, 0x9200)]
    rec = Recorder()
    K.reduce_group(rec, ST, entries)
    _expect(rec, "ltrx_reduce_group", n=3, src=[0x1000, 0x2000, 0x3000], splits=[5, 4, 6], row_stride=[240, 20, 24], cols=[240, 20, 12],
            dst=[0x9000, 0x9100, 0x9200], stream=ST.value)


def test_input_norm_and_positional_encoding_calls():
    x, w, b, y, mean, rstd = f32(9, 12), f32(12), f32(12), f32(9, 12), f32(9), f32(9)
    rec = Recorder()
    K.layernorm_torch_fwd(rec, ST, x, w, b, 7, 1e-5, y, mean, rstd)
    _expect(rec, "ltrx_layernorm_torch_fwd", x=x.data_ptr(), w=w.data_ptr(), b=b.data_ptr(), rows=7, D=12, eps=1e-5, y=y.data_ptr(),
            mean_out=mean.data_ptr(), rstd_out=rstd.data_ptr(), stream=ST.value)
    xs, ys = f32(9, 16)[:, :12], f32(9, 32)[:, :12]                                   # the padded operand rows
    rec = Recorder()
    K.layernorm_torch_fwd_strided(rec, ST, xs, w, b, 7, 1e-5, ys, mean, rstd)
    _expect(rec, "ltrx_layernorm_torch_fwd_strided", x=xs.data_ptr(), ldx=16, w=w.data_ptr(), b=b.data_ptr(), rows=7, D=12, eps=1e-5,
            y=ys.data_ptr(), ldy=32, mean_out=mean.data_ptr(), rstd_out=rstd.data_ptr(), stream=ST.value)
    table, idx, mask = f32(50, 12), i64(9), u8(9)
    rec = Recorder()
    K.posenc_fwd(rec, ST, x, table, idx, mask, 7, 49, 3.5, y)
    _expect(rec, "ltrx_posenc_fwd", x=x.data_ptr(), table=table.data_ptr(), indices=idx.data_ptr(), mask=mask.data_ptr(), M=7, D=12,
            padding_idx=49, scale=3.5, y=y.data_ptr(), stream=ST.value)
    rec = Recorder()
    K.posenc_table_bwd(rec, ST, x, idx, None, 7, 49, table)                           # packed rows: no key mask
    _expect(rec, "ltrx_posenc_table_bwd", dx=x.data_ptr(), indices=idx.data_ptr(), mask=None, M=7, D=12, padding_idx=49,
            dtable=table.data_ptr(), stream=ST.value)


@pytest.mark.parametrize("with_y", [False, True])
def test_norm_head_calls(with_y):
    x, a, b, w, bias, sc, mean, rstd = f32(9, 12), f32(12), f32(12), f32(1, 12), f32(1), f32(9), f32(9), f32(9)
    y = f32(9, 12) if with_y else None
    rec = Recorder()
    K.norm_head_fwd(rec, ST, x, a, b, w, bias, 7, 1e-6, sc, mean, rstd, *((y,) if with_y else ()))
    _expect(rec, "ltrx_norm_head_fwd", x=x.data_ptr(), a=a.data_ptr(), b=b.data_ptr(), w=w.data_ptr(), bias=bias.data_ptr(), rows=7, D=12,
            eps=1e-6, scores_out=sc.data_ptr(), mean_out=mean.data_ptr(), rstd_out=rstd.data_ptr(), y_out=y.data_ptr() if with_y else None,
            stream=ST.value)
    ds, dw, db, dx, ws = f32(9), f32(1, 12), f32(1), f32(9, 12), u8(64)
    rec = Recorder()
    K.norm_head_wgrad(rec, ST, ds, x, a, b, mean, rstd, 7, dw, db, ws)
    _expect(rec, "ltrx_norm_head_wgrad", dscores=ds.data_ptr(), xsum=x.data_ptr(), a=a.data_ptr(), b=b.data_ptr(), mean=mean.data_ptr(),
            rstd=rstd.data_ptr(), M=7, D=12, dw=dw.data_ptr(), db=db.data_ptr(), ws=ws.data_ptr(), stream=ST.value)
    rec = Recorder(rows_out=5)
    assert K.norm_head_bwd_partial(rec, ST, ds, x, a, w, mean, rstd, 7, 1e-6, dx, ws) == 5
    _expect(rec, "ltrx_norm_head_bwd_partial", dscores=ds.data_ptr(), xsum=x.data_ptr(), a=a.data_ptr(), w=w.data_ptr(),
            mean=mean.data_ptr(), rstd=rstd.data_ptr(), rows=7, D=12, eps=1e-6, dx_out=dx.data_ptr(), ws=ws.data_ptr(),
            partial_rows_out="byref", stream=ST.value)


def test_optimizer_calls():
    p, g, m, v, step, scale, norm, ws = f32(40), f32(40), f32(40), f32(40), f32(1), f32(1), f32(1), u8(64)
    rec = Recorder()
    K.clip_grad_norm_scale(rec, ST, g, 0.5, scale, norm, ws)
    _expect(rec, "ltrx_clip_grad_norm_scale", grads=g.data_ptr(), n=40, max_norm=0.5, scale_out=scale.data_ptr(), norm_out=norm.data_ptr(),
            ws=ws.data_ptr(), stream=ST.value)
    rec = Recorder(returns={"ltrx_clip_workspace_bytes": 256})
    assert K.clip_workspace(rec, 40, g).numel() == 256
    _expect(rec, "ltrx_clip_workspace_bytes", n=40)
    adam = dict(params=p.data_ptr(), grads=g.data_ptr(), exp_avg=m.data_ptr(), exp_avg_sq=v.data_ptr(), n=40, lr=1e-3, beta1=0.9,
                beta2=0.999, eps=1e-8, weight_decay=0.01, step_count=step.data_ptr(), grad_scale=1.0, stream=ST.value)
    rec = Recorder()
    K.adam_step(rec, ST, p, g, m, v, 1e-3, (0.9, 0.999), 1e-8, 0.01, True, step, scale)     # AdamW behind the clip: its device scale
    _expect(rec, "ltrx_adam_step", decoupled=1, grad_scale_dev=scale.data_ptr(), **adam)
    rec = Recorder()
    K.adam_step(rec, ST, p, g, m, v, 1e-3, (0.9, 0.999), 1e-8, 0.01, False, step)
    _expect(rec, "ltrx_adam_step", decoupled=0, grad_scale_dev=None, **adam)
    sgd = dict(params=p.data_ptr(), grads=g.data_ptr(), n=40, lr=0.01, weight_decay=0.02, grad_scale=1.0, stream=ST.value)
    rec = Recorder()
    K.sgd_step(rec, ST, p, g, m, 0.01, 0.9, True, 0.02, scale)
    _expect(rec, "ltrx_sgd_step", momentum_buf=m.data_ptr(), momentum=0.9, nesterov=1, grad_scale_dev=scale.data_ptr(), **sgd)
    rec = Recorder()
    K.sgd_step(rec, ST, p, g, None, 0.01, 0.0, False, 0.02)                           # no momentum: no buffer
    _expect(rec, "ltrx_sgd_step", momentum_buf=None, momentum=0.0, nesterov=0, grad_scale_dev=None, **sgd)
    seg, out = i64(5), i32(2)
    rec = Recorder()
    K.first_nonfinite(rec, ST, g, seg, out)
    _expect(rec, "ltrx_first_nonfinite", buf=g.data_ptr(), n=40, seg_start=seg.data_ptr(), n_seg=5, out=out.data_ptr(), stream=ST.value)


@pytest.mark.parametrize("extras", [True, False])
def test_fc_listnet_step_calls(extras):
    """``extras``: the optimizer block, ``hidden`` and ``dscores`` are passed -- or all left out (NULL pointers, zero scalars)"""
    B, L, F, H = 3, 5, 12, 8
    x, y, params, grads, m, v, step = f32(B * L, F), f32(B, L), f32(200), f32(200), f32(200), f32(200), f32(1)
    scores, dsc, hid, loss, ws = f32(B, L), f32(B, L), f32(B * L, H), f32(1), u8(64)
    opt = (m, v, step, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0) if extras else None
    common = dict(x=x.data_ptr(), y=y.data_ptr(), B=B, L=L, F=F, H=H, params=params.data_ptr(), off_w1=4, off_b1=100, off_wout=108,
                  off_bout=116, nflat=200, eps=1e-10, pad_value=-1.0, batch_divisor=6.0, scores=scores.data_ptr(),
                  dscores=dsc.data_ptr() if extras else None, loss_out=loss.data_ptr(), grads=grads.data_ptr(),
                  exp_avg=m.data_ptr() if extras else None, exp_avg_sq=v.data_ptr() if extras else None,
                  step_count=step.data_ptr() if extras else None, lr=1e-3 if extras else 0.0, beta1=0.9 if extras else 0.0,
                  beta2=0.999 if extras else 0.0, adam_eps=1e-8 if extras else 0.0, weight_decay=0.01 if extras else 0.0, decoupled=0,
                  ws=ws.data_ptr(), stream=ST.value)
    rec = Recorder()
    K.fc_listnet_step(rec, ST, x, y, B, L, H, 1, params, 4, 100, 108, 116, 1e-10, -1, 6.0, scores, loss, grads, ws, opt,
                      hid if extras else None, dsc if extras else None)
    _expect(rec, "ltrx_fc_listnet_step", act=1, hidden_out=hid.data_ptr() if extras else None, **common)
    rec = Recorder()
    K.fc_linear_listnet_step(rec, ST, x, y, B, L, H, params, 4, 100, 108, 116, 1e-10, -1, 6.0, scores, loss, grads, ws, opt,
                             dsc if extras else None)
    _expect(rec, "ltrx_fc_linear_listnet_step", **common)
    rec = Recorder(returns={"ltrx_fc_listnet_workspace_bytes": 2048})
    assert K.fc_listnet_workspace(rec, B, L, F, H, 200, x).numel() == 2048
    _expect(rec, "ltrx_fc_listnet_workspace_bytes", B=B, L=L, F=F, H=H, nflat=200)
    rec = Recorder(returns={"ltrx_fc_linear_listnet_workspace_bytes": 96})
    assert K.fc_linear_listnet_workspace(rec, B, F, x).numel() == 96
    _expect(rec, "ltrx_fc_linear_listnet_workspace_bytes", B=B, F=F)


# ------------------------------------------------------------------------------------------------------------------
# ranking, clicks, the MFMA self-test
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["grid", "resident"])
def test_rank_slates_cu(source):
    import types
    from allrank_amd import inference
    assert inference.rank_slates_cu is K.rank_slates_cu and "rank_slates_cu" in inference.__all__
    B, L, F, ml = 3, 7, 12, 5
    scores, cu, order, perm = f32(11), i32(B + 1), i32(B), i32(11)
    x, y, x_out, y_out = f32(B, L, F), f32(B, L), f32(B, L, F), f32(B, L)
    slates, ids = types.SimpleNamespace(x_items=f32(40, F), y_items=f32(40), offsets=i64(9)), i64(B)
    grid = source == "grid"
    rec = Recorder()
    if grid:
        K.rank_slates_cu(rec, ST, scores, cu, order, B, ml, L, x_out, y_out, perm, x=x, y=y)
    else:
        K.rank_slates_cu(rec, ST, scores, cu, None, B, ml, L, x_out, y_out, slates=slates, ids=ids)
    _expect(rec, "ltrx_rank_slates_cu", scores=scores.data_ptr(), x=x.data_ptr() if grid else None, y=y.data_ptr() if grid else None,
            x_items=None if grid else slates.x_items.data_ptr(), y_items=None if grid else slates.y_items.data_ptr(),
            offsets=None if grid else slates.offsets.data_ptr(), ids=None if grid else ids.data_ptr(), cu_seqlens=cu.data_ptr(),
            slate_order=order.data_ptr() if grid else None, B=B, max_len=ml, F=F, L=L, perm=perm.data_ptr() if grid else None,
            x_out=x_out.data_ptr(), y_out=y_out.data_ptr(), stream=ST.value)


@pytest.mark.parametrize("optional", [True, False])
def test_click_slates_cu(optional):
    """``optional``: ``u``, ``observe_p``, ``margin_out`` and ``ws`` are passed, or all NULL.  ``q_host`` is the address of a double
    that holds the plan's q while the call runs"""
    from allrank_amd import clicks
    assert clicks.click_slates_cu is K.click_slates_cu
    B, L, F, ml = 3, 7, 12, 5
    x, y, cu, order, out = f32(B, L, F), f32(B, L), i32(B + 1), i32(B), f32(B, L)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64)  # noqa: E731
    u, table, mg, ws = (f64(11), f64(L), f64(B), u8(64)) if optional else (None, None, None, None)
    plan = dict(kind="cascade", eta=1, threshold=2.0, max_candidates=4, diverse=1, q=0.25, max_clicks=6)
    rec = Recorder(reads={"q_host": ctypes.c_double})
    K.click_slates_cu(rec, ST, x, y, cu, order, B, ml, out, plan, u, table, mg, ws)
    at = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _expect(rec, "ltrx_click_slates_cu", x=x.data_ptr(), y=y.data_ptr(), cu_seqlens=cu.data_ptr(), slate_order=order.data_ptr(), B=B,
            max_len=ml, F=F, L=L, u=at(u), observe_p=at(table), threshold=2.0, max_candidates=4, diverse=1, q_host=0.25, max_clicks=6,
            clicks_out=out.data_ptr(), margin_out=at(mg), ws=at(ws), stream=ST.value)


def test_selftest_mfma():
    A, B, D = f32(32, 2), f32(2, 32), f32(32, 32)
    rec = Recorder()
    K.selftest_mfma32x32x2(rec, ST, A, B, D)
    _expect(rec, "ltrx_selftest_mfma32x32x2", A=A.data_ptr(), B=B.data_ptr(), D=D.data_ptr(), stream=ST.value)


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
    # the scan sees the launchers' calls, the queries the engine keeps and the loss, metric and loader launchers
    assert {"ltrx_gemm_nt", "ltrx_mha_bwd", "ltrx_norm_head_fwd", "ltrx_weight_images", "ltrx_fc_listnet_step", "ltrx_listnet_fwd_bwd",
            "ltrx_adam_step"} <= seen and len(seen) >= 60, sorted(seen)


def _is_query(name):
    """capability predicates, byte counts and the plan hooks launch nothing: a caller may ask them directly"""
    return name.endswith(("_supported", "_bytes")) or name.startswith("ltrx_debug_")


LAUNCHED_THROUGH_KERNELS = ("engine.py", "ops.py", "rows.py", "inference.py", "clicks.py", "fit.py")


def test_each_launched_call_is_written_once():
    """every launch kernels.py states appears nowhere else in the package, the modules that launch through kernels.py state none of
    their own (a query may stay: the engine sizes one workspace for the largest of several shapes), and every launch kernels.py
    states has a marshalling test in this module"""
    kernels_py = os.path.join("allrank_amd", "kernels.py")
    mine = {node.func.attr for path, node in _ltrx_calls() if path == kernels_py and not _is_query(node.func.attr)}
    count = {}
    for path, node in _ltrx_calls():
        if node.func.attr in mine:
            count[node.func.attr] = count.get(node.func.attr, 0) + 1
    assert set(count.values()) == {1}, {k: v for k, v in count.items() if v != 1}
    stray = [(path, node.lineno, node.func.attr) for path, node in _ltrx_calls()
             if path in [os.path.join("allrank_amd", m) for m in LAUNCHED_THROUGH_KERNELS] and not _is_query(node.func.attr)]
    assert not stray, stray
    assert mine >= {"ltrx_gemm_nt", "ltrx_gemm_tn", "ltrx_mha_fwd", "ltrx_mha_bwd", "ltrx_layernorm_fwd", "ltrx_layernorm_bwd",
                    "ltrx_layernorm_bwd_partial", "ltrx_score_head_fwd", "ltrx_score_head_bwd", "ltrx_out_act_fwd", "ltrx_out_act_bwd",
                    "ltrx_split_image", "ltrx_gather_rows_cu",
                    # the packing calls
                    "ltrx_gather_rows", "ltrx_scatter_rows", "ltrx_packed_row_index", "ltrx_scatter_rows_cu", "ltrx_zero_rows_cu",
                    "ltrx_assemble_packed", "ltrx_ingest_batch",
                    # the training step's own calls
                    "ltrx_dropout_apply", "ltrx_colsum", "ltrx_relu_bwd", "ltrx_weight_images", "ltrx_transpose_batch",
                    "ltrx_gemm_tn_group", "ltrx_gemm_tn_group_ln", "ltrx_reduce_group", "ltrx_layernorm_torch_fwd",
                    "ltrx_layernorm_torch_fwd_strided", "ltrx_posenc_fwd", "ltrx_posenc_table_bwd", "ltrx_scale_inplace",
                    "ltrx_norm_head_fwd", "ltrx_norm_head_wgrad", "ltrx_norm_head_bwd_partial", "ltrx_clip_grad_norm_scale",
                    "ltrx_sgd_step", "ltrx_adam_step", "ltrx_bump_u32", "ltrx_first_nonfinite", "ltrx_fc_listnet_step",
                    "ltrx_fc_linear_listnet_step",
                    # ranking, clicks, the MFMA self-test
                    "ltrx_rank_slates_cu", "ltrx_click_slates_cu", "ltrx_selftest_mfma32x32x2"}, sorted(mine)
    with open(os.path.abspath(__file__)) as fh:
        tree = ast.parse(fh.read())
    tested = {node.args[1].value for node in ast.walk(tree)
              if isinstance(node, ast.Call) and getattr(node.func, "id", "") == "_expect" and isinstance(node.args[1], ast.Constant)}
    assert mine <= tested, sorted(mine - tested)
