"""The one Python statement of each scoring-model kernel call of libltrx.so (include/ltrx.h): GEMMs, attention, LayerNorm, score
head, output activation, weight images and the packing calls -- batch ingest, the index layout's ``gather_rows`` / ``scatter_rows`` /
``packed_row_index``, the cu_seqlens layout's ``gather_rows_cu`` / ``scatter_rows_cu`` / ``zero_rows_cu`` / ``assemble_packed``.  The
autograd bindings (allrank_amd/ops.py), the explicit training step (allrank_amd/engine.py) and the row movers (allrank_amd/rows.py)
launch through these functions, as the plugin losses and ``FusedLoss`` launch through the ``_launch_*`` functions of
allrank_amd/losses.

A launcher makes exactly ONE ``ltrx_*`` call on the tensors it is handed.  Shapes, row strides and the head width are read from the
tensors (an operand may be a column-slice view of a wider buffer: its ``data_ptr()`` and ``stride`` say where it lives), so no caller
restates them or adds byte offsets to an address.  A launcher allocates nothing, checks no device, makes nothing contiguous and looks
up no stream: the bound library ``lib`` and the stream ``st`` are arguments, which is what lets tests/test_kernel_calls_cpu.py hold
every call to the header's parameter names with CPU tensors and a recording stand-in for the library.  The ``*_workspace`` helpers
are the exception that allocates: they ask the library for the byte count and return ``_lib.workspace`` of it.
"""
import ctypes

from ._lib import check, ptr as P, workspace


# ---- dense projections ---------------------------------------------------------------------------------------------
def gemm_nt(lib, st, a, b, out, rows, bias=None, act=0, aux=None, p=0.0, seed=0, drop_step=None, prec=0, tile=0, b_image=None,
            what="gemm_nt"):
    """out[:rows] = epi_act(a[:rows] b^T + bias), dropout (p, site ``seed``, step word ``drop_step``) in the epilogue; ``aux`` as the
    act code reads it: a float matrix with its own row stride (acts 2 / 3), or the one-bit ReLU mask buffer (acts 4 / 5: no stride).
    ``b_image``: the address of ``b``'s pre-split image (ltrx_split_image) or None."""
    ldaux = 0 if aux is None or act in (4, 5) else aux.stride(0)
    check(lib.ltrx_gemm_nt(P(a), a.stride(0), P(b), b.stride(0), b_image, P(out), out.stride(0), rows, b.shape[0], a.shape[1], P(bias),
                           act, P(aux), ldaux, float(p), seed, P(drop_step), prec, tile, st), what)


def gemm_tn_workspace(lib, rows, N, K, like):
    return workspace(lib.ltrx_gemm_tn_workspace_bytes(rows, N, K), like)


def gemm_tn(lib, st, dy, x, gw, gb, rows, prec, tile, ws, what="gemm_tn"):
    """gw = dy[:rows]^T x[:rows], gb (may be None) = column sums of dy[:rows]"""
    check(lib.ltrx_gemm_tn(P(dy), dy.stride(0), P(x), x.stride(0), P(gw), P(gb), rows, dy.shape[1], x.shape[1], prec, tile, P(ws), st),
          what)


# ---- attention: q / k / v (dq / dk / dv) are [..., rows, h * d_k] tensors or column-slice views that share one row stride ----
def thirds(t):
    """the q | k | v (dq | dk | dv) column blocks of a packed projection [..., 3 h d_k], as views"""
    d = t.shape[-1] // 3
    return t[..., :d], t[..., d:2 * d], t[..., 2 * d:]


def mha_fwd(lib, st, q, k, v, kpm, B, L, h, o, lse, p, seed, drop_step, cu, order, mode):
    check(lib.ltrx_mha_fwd(P(q), P(k), P(v), P(kpm), B, L, h, q.shape[-1] // h, q.stride(-2), P(o), o.stride(-2), P(lse), float(p), seed,
                           P(drop_step), P(cu), P(order), mode, st), "mha_fwd")


def mha_bwd_workspace(lib, B, L, h, d_k, mode, like):
    return workspace(lib.ltrx_mha_bwd_workspace_bytes(B, L, h, d_k, mode), like)


def mha_bwd(lib, st, q, k, v, kpm, o, do, lse, B, L, h, dq, dk, dv, p, seed, drop_step, cu, order, mode, ws):
    check(lib.ltrx_mha_bwd(P(q), P(k), P(v), P(kpm), P(o), P(do), P(lse), B, L, h, q.shape[-1] // h, q.stride(-2), o.stride(-2), P(dq),
                           P(dk), P(dv), dq.stride(-2), float(p), seed, P(drop_step), P(cu), P(order), mode, P(ws), st), "mha_bwd")


# ---- LayerNorm (transformer.py:73-81) over rows of x.shape[-1] columns -----------------------------------------------
def layernorm_fwd(lib, st, x, res, a, b, rows, eps, xsum, y, mean, rstd, p=0.0, seed=0, drop_step=None):
    """y = LN(x + drop_p(res)); xsum (may be None) = x + drop_p(res)"""
    check(lib.ltrx_layernorm_fwd(P(x), P(res), P(a), P(b), rows, x.shape[-1], float(eps), P(xsum), P(y), P(mean), P(rstd), float(p), seed,
                                 P(drop_step), st), "layernorm_fwd")


def layernorm_bwd_workspace(lib, rows, D, like):
    return workspace(lib.ltrx_layernorm_bwd_workspace_bytes(rows, D), like)


def layernorm_bwd(lib, st, dy, xsum, a, mean, rstd, dres, rows, eps, dx, da, db, ws, what="layernorm_bwd"):
    check(lib.ltrx_layernorm_bwd(P(dy), P(xsum), P(a), P(mean), P(rstd), P(dres), rows, xsum.shape[-1], float(eps), P(dx), P(da), P(db),
                                 P(ws), st), what)


def layernorm_bwd_partial(lib, st, dy, xsum, a, mean, rstd, dres, rows, eps, dx, ws):
    """dx now; returns how many rows of [da | db] partials the call left in ``ws`` for the caller to sum"""
    rows_out = ctypes.c_int(0)
    check(lib.ltrx_layernorm_bwd_partial(P(dy), P(xsum), P(a), P(mean), P(rstd), P(dres), rows, xsum.shape[-1], float(eps), P(dx), P(ws),
                                         ctypes.byref(rows_out), st), "layernorm_bwd_partial")
    return rows_out.value


# ---- OutputLayer with d_output == 1 (model.py:111-117) and the elementwise activations -------------------------------
def score_head_fwd(lib, st, x, w, b, rows, scores):
    check(lib.ltrx_score_head_fwd(P(x), P(w), P(b), rows, x.shape[-1], P(scores), st), "score_head_fwd")


def score_head_bwd_workspace(lib, rows, D, like):
    return workspace(lib.ltrx_score_head_bwd_workspace_bytes(rows, D), like)


def score_head_bwd(lib, st, ds, x, w, rows, dx, dw, db, ws):
    check(lib.ltrx_score_head_bwd(P(ds), P(x), P(w), rows, x.shape[-1], P(dx), P(dw), P(db), P(ws), st), "score_head_bwd")


def out_act_fwd(lib, st, z, n, kind, y, what="out_act_fwd"):
    """y[:n] = act(z[:n]) elementwise, kind 1 = Sigmoid, 2 = Tanh (in place where y is z)"""
    check(lib.ltrx_out_act_fwd(P(z), n, kind, P(y), st), what)


def out_act_bwd(lib, st, dy, y, n, kind, dz, what="out_act_bwd"):
    """dz[:n] = dy[:n] * act'(.) taken from the stored output y"""
    check(lib.ltrx_out_act_bwd(P(dy), P(y), n, kind, P(dz), st), what)


# ---- weight images ---------------------------------------------------------------------------------------------------
def split_image(lib, st, src, dst, what="split_image"):
    """dst = the pre-split bf16 hi / lo image of every float of ``src`` (same offsets)"""
    check(lib.ltrx_split_image(P(src), P(dst), src.numel(), st), what)


# ---- packing: batches into the step's buffers, values between the packed rows and the padded [B, L] grid -----------------
def _ld(t, cols):
    """row stride of ``t`` read as rows of ``cols`` floats: a [rows, cols] matrix -- a column slice of a wider buffer included -- says
    its own; any other shape ([B, L] scores of one column, [B, L, cols], a vector of one column) is a dense grid of such rows"""
    return t.stride(0) if t.dim() == 2 and t.shape[1] == cols else cols


def ingest_batch(lib, st, x, y, pad_value, x_dst, y_dst, mask_dst):
    """y_dst = y, mask_dst = (y == pad_value) and the rows of ``x`` into the rows of ``x_dst`` (F columns each, its own row stride) in
    one launch.  ``x`` None (the packed layouts gather the features themselves): labels and mask only -- ``x_dst`` then still
    states the row shape, and nothing is written to it."""
    check(lib.ltrx_ingest_batch(P(x), P(y), 0 if x is None else x.numel(), y.numel(), x_dst.shape[1], x_dst.stride(0), float(pad_value),
                                None if x is None else P(x_dst), P(y_dst), P(mask_dst), st), "ingest_batch")


def packed_row_index(lib, st, cu, B, L, n, idx):
    """idx[r] = b * L + (r - cu[b]) for packed row r < n of slate b (valid items first in every slate)"""
    check(lib.ltrx_packed_row_index(P(cu), B, L, n, P(idx), st), "packed_row_index")


def gather_rows(lib, st, src, idx, n, n_pad, cols, dst, what="gather_rows"):
    """dst[r] = row idx[r] of ``src`` for r < n, rows n .. n_pad-1 of ``dst`` zero (``cols`` floats per row; strides: ``_ld``)"""
    check(lib.ltrx_gather_rows(P(src), _ld(src, cols), P(idx), n, n_pad, cols, P(dst), _ld(dst, cols), st), what)


def scatter_rows(lib, st, src, idx, n, cols, dst):
    """row idx[r] of ``dst`` = src[r] for r < n (the inverse of ``gather_rows``; the other rows of ``dst`` stay)"""
    check(lib.ltrx_scatter_rows(P(src), _ld(src, cols), P(idx), n, cols, P(dst), _ld(dst, cols), st), "scatter_rows")


def assemble_packed(lib, st, x_items, y_items, offsets, slates, cu, B, L, rows, x_out, y_out, idx_out, pos_out=None):
    """the slates ``slates`` (device int64 ids) of a resident CSR set straight into packed rows: features into ``x_out`` [rows, F] (a
    view with its own row stride; alignment rows 0), padded labels into ``y_out`` [B, L], the packed-row index, and -- ``pos_out`` --
    the int64 position of every row (alignment rows: -1)"""
    check(lib.ltrx_assemble_packed(P(x_items), P(y_items), P(offsets), P(slates), P(cu), B, L, x_out.shape[1], rows, P(x_out),
                                   x_out.stride(0), P(y_out), P(idx_out), P(pos_out), st), "assemble_packed")


def scatter_rows_cu(lib, st, src, cu, B, L, cols, rows, dst):
    """the packed rows ``src`` -> the padded grid ``dst`` [B, L] of ``cols`` floats per item, 0 on padded slots; the valid count is
    read from the device ``cu``"""
    check(lib.ltrx_scatter_rows_cu(P(src), _ld(src, cols), P(cu), B, L, cols, rows, P(dst), _ld(dst, cols), st), "scatter_rows_cu")


def zero_rows_cu(lib, st, x, cu, B, rows):
    """x[cu[B] : rows] = 0, the count read on the device (the launch is the same for every batch of a row bucket)"""
    check(lib.ltrx_zero_rows_cu(P(x), x.stride(0), x.shape[1], P(cu), B, rows, st), "zero_rows_cu")


def gather_rows_cu(lib, st, src, cu, B, L, cols, rows, dst, idx_out=None, what="gather_rows_cu"):
    """the valid items of the dense padded grid ``src`` [slates, L] of ``cols`` 4-byte words per item -> consecutive rows of ``dst``,
    the valid count read from the device ``cu``; an int64 tensor moves as pairs of words (cols 2, and a row stride counted in words)"""
    check(lib.ltrx_gather_rows_cu(P(src), cols, P(cu), B, L, cols, rows, P(dst), dst.stride(0) * (dst.element_size() // 4), P(idx_out),
                                  st), what)
