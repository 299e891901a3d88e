"""The one Python statement of each kernel call of libltrx.so (include/ltrx.h) outside the losses, the metrics, the data loader and the
feature normalisation of resident data (allrank_amd/normalize.py states its three calls in this module's form):
  * the scoring model: GEMMs, attention, LayerNorm, score head, output activation, weight images;
  * the packing calls: batch ingest, the index layout's ``gather_rows`` / ``scatter_rows`` / ``packed_row_index``, the cu_seqlens
    layout's ``gather_rows_cu`` / ``scatter_rows_cu`` / ``zero_rows_cu`` / ``assemble_packed``;
  * the training step's own calls: dropout plumbing, column sums, the ReLU backward, the weight-image refresh, the grouped weight
    gradient (with and without the LayerNorm backward at its side) and the grouped reduction, the input norm, the positional
    encoding, the fused norm + head, clip / SGD / Adam, the finiteness check and the two slate-resident FC + ListNet steps;
  * ranking and clicks: ``rank_slates_cu``, ``click_slates_cu``; and the MFMA lane-layout self-test.
The autograd bindings (allrank_amd/ops.py), the explicit training step (allrank_amd/engine.py), the row movers (allrank_amd/rows.py),
allrank_amd/inference.py and allrank_amd/clicks.py launch through these functions and state no launch of their own, as the plugin
losses and ``FusedLoss`` launch through the ``_launch_*`` functions of allrank_amd/losses.

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


# ---- the training step's own calls: elementwise plumbing -------------------------------------------------------------
def bump_u32(lib, st, word):
    """word[0] += 1: the per-step word folded into every dropout seed (a replayed hipGraph re-keys its masks)"""
    check(lib.ltrx_bump_u32(P(word), st), "bump_u32")


def dropout_apply(lib, st, src, rows, p, seed, drop_step, dst):
    """dst[:rows] = src[:rows] * keep-mask / (1 - p) of the site ``seed`` (in place where dst is src)"""
    check(lib.ltrx_dropout_apply(P(src), P(dst), rows * src.shape[1], float(p), seed, P(drop_step), st), "dropout_apply")


def colsum_workspace(lib, rows, N, like):
    return workspace(lib.ltrx_colsum_workspace_bytes(rows, N), like)


def colsum(lib, st, a, rows, out, ws):
    """out = column sums of a[:rows] (not accumulated)"""
    check(lib.ltrx_colsum(P(a), rows, a.shape[1], a.stride(0), P(out), 0, P(ws), st), "colsum")


def relu_bwd(lib, st, dr, r, rows, scale):
    """dr[:rows] *= (r > 0) * scale: backward of dropout(relu(z)) from the stored post-dropout activation ``r``"""
    check(lib.ltrx_relu_bwd(P(dr), P(r), rows * dr.shape[1], scale, st), "relu_bwd")


def scale_inplace(lib, st, x, n, s):
    check(lib.ltrx_scale_inplace(P(x), n, s, st), "scale_inplace")


# ---- weight images and transposed copies of the flat parameter buffer ------------------------------------------------------
def weight_images(lib, st, src, src_image, dst, dst_image, desc, tile_start, n, total_tiles, pad_src=None, pad_dst=None,
                  pad_dst_image=None):
    """the image of ``src``, the ``n`` transposed copies ``desc`` describes in ``dst`` and their image in one launch; ``pad_src``
    [rows, cols] (optional) also lands in ``pad_dst`` (rows of its own, wider stride) with its image in ``pad_dst_image``"""
    pad = (0, 0, 0) if pad_src is None else (pad_src.shape[0], pad_src.shape[1], pad_dst.stride(0))
    check(lib.ltrx_weight_images(P(src), src.numel(), P(src_image), P(dst), P(dst_image), P(desc), P(tile_start), n, total_tiles,
                                 P(pad_src), pad[0], pad[1], pad[2], P(pad_dst), P(pad_dst_image), st), "weight_images")


def transpose_batch(lib, st, src, dst, desc, tile_start, n, total_tiles):
    check(lib.ltrx_transpose_batch(P(src), P(dst), P(desc), P(tile_start), n, total_tiles, st), "transpose_batch")


# ---- the grouped weight gradient: ``problems`` = [(dy, x, gw, gb)], gw_i = dy_i[:rows]^T x_i[:rows], gb_i = column sums of dy_i ----
def _tn_group(problems):
    """(nprob, A, lda, B, ldb, C, bias_out, NP, KP): the ctypes arrays of the group's operands, strides and shapes"""
    n = len(problems)
    vp, ci = ctypes.c_void_p * n, ctypes.c_int * n
    return (n, vp(*[t[0].data_ptr() for t in problems]), ci(*[t[0].stride(0) for t in problems]),
            vp(*[t[1].data_ptr() for t in problems]), ci(*[t[1].stride(0) for t in problems]),
            vp(*[t[2].data_ptr() for t in problems]), vp(*[t[3].data_ptr() for t in problems]),
            ci(*[t[0].shape[1] for t in problems]), ci(*[t[1].shape[1] for t in problems]))


def _tn_slabs(n, defer):
    """the by-reference outputs of a deferred reduction (NULL x 3 otherwise), and what the caller reads of them after the call"""
    if not defer:
        return (None, None, None), lambda: None
    so, bso, sp = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(), ctypes.c_int(0)
    return (so, bso, ctypes.byref(sp)), lambda: (list(so), list(bso), sp.value)


def tn_group_plan(lib, problems, rows, prec, ws):
    """does the grouped kernel take this composition with this workspace (the library's own host-side predicate), or does the call
    run one launch per problem?"""
    n, _, lda, _, ldb, _, _, NP, KP = _tn_group(problems)
    return bool(lib.ltrx_debug_tn_group_plan(n, rows, NP, KP, lda, ldb, prec, ws.numel(), ctypes.byref(ctypes.c_int(0)),
                                             ctypes.byref(ctypes.c_size_t(0))))


def gemm_tn_group(lib, st, problems, rows, prec, ws, defer=False, what="gemm_tn_group"):
    """every problem in one launch.  ``defer``: the partial slabs stay in ``ws`` for the caller's reducing launch; returns (slab
    address per problem, bias-slab address -- or None -- per problem, split count: 0 = nothing left to reduce), else None"""
    n, A, lda, B, ldb, C, bo, NP, KP = _tn_group(problems)
    outs, result = _tn_slabs(n, defer)
    check(lib.ltrx_gemm_tn_group(n, A, lda, B, ldb, C, bo, rows, NP, KP, prec, P(ws), ws.numel(), outs[0], outs[1], outs[2], st), what)
    return result()


def gemm_tn_group_ln(lib, st, problems, rows, prec, ws, dy, xsum, a, mean, rstd, dres, eps, dx, ln_ws, defer=False,
                     what="gemm_tn_group_ln"):
    """``gemm_tn_group`` and ``layernorm_bwd_partial(dy .. ln_ws)`` over the same rows in ONE call (the LayerNorm backward in the
    launch's idle CUs where the library takes it).  Returns (what ``gemm_tn_group`` returns, rows of [da | db] partials left in
    ``ln_ws``, side workgroups used: 0 = two launches)"""
    n, A, lda, B, ldb, C, bo, NP, KP = _tn_group(problems)
    outs, result = _tn_slabs(n, defer)
    rows_out, side = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.ltrx_gemm_tn_group_ln(n, A, lda, B, ldb, C, bo, rows, NP, KP, prec, P(ws), ws.numel(), outs[0], outs[1], outs[2], P(dy),
                                    P(xsum), P(a), P(mean), P(rstd), P(dres), rows, xsum.shape[-1], float(eps), P(dx), P(ln_ws),
                                    ctypes.byref(rows_out), 0, ctypes.byref(side), st), what)
    return result(), rows_out.value, side.value


def reduce_group(lib, st, entries):
    """dst = the fixed-order sum of ``partial rows`` rows of ``columns`` floats, ``row stride`` apart, from src -- for every (src
    address, partial rows, row stride, columns, dst address) of ``entries``, in one launch"""
    n = len(entries)
    vp, cs = ctypes.c_void_p * n, ctypes.c_size_t * n
    check(lib.ltrx_reduce_group(n, vp(*[e[0] for e in entries]), (ctypes.c_int * n)(*[e[1] for e in entries]), cs(*[e[2] for e in entries]),
                                cs(*[e[3] for e in entries]), vp(*[e[4] for e in entries]), st), "reduce_group")


# ---- around the encoder: FCModel.input_norm (nn.LayerNorm), the positional encoding, the fused final norm + score head ----------
def layernorm_torch_fwd(lib, st, x, w, b, rows, eps, y, mean, rstd):
    """y = nn.LayerNorm(x) over dense rows of w.numel() columns"""
    check(lib.ltrx_layernorm_torch_fwd(P(x), P(w), P(b), rows, w.numel(), float(eps), P(y), P(mean), P(rstd), st), "layernorm_torch_fwd")


def layernorm_torch_fwd_strided(lib, st, x, w, b, rows, eps, y, mean, rstd):
    """the same rows, read and written at the operands' own row strides (column slices of padded buffers)"""
    check(lib.ltrx_layernorm_torch_fwd_strided(P(x), x.stride(0), P(w), P(b), rows, w.numel(), float(eps), P(y), y.stride(0), P(mean),
                                               P(rstd), st), "layernorm_torch_fwd_strided")


def posenc_fwd(lib, st, x, table, indices, mask, rows, padding_idx, scale, y):
    """y = scale * x + table[indices] (transformer.py:51-52); ``mask`` (may be None): rows that take the padding index"""
    check(lib.ltrx_posenc_fwd(P(x), P(table), P(indices), P(mask), rows, x.shape[1], padding_idx, scale, P(y), st), "posenc_fwd")


def posenc_table_bwd(lib, st, dx, indices, mask, rows, padding_idx, dtable):
    """dtable = the gradient of a learned table: the rows of ``dx`` summed per index"""
    check(lib.ltrx_posenc_table_bwd(P(dx), P(indices), P(mask), rows, dx.shape[1], padding_idx, P(dtable), st), "posenc_table_bwd")


def norm_head_fwd(lib, st, x, a, b, w, bias, rows, eps, scores, mean, rstd, y=None):
    """scores = LN(x) w + bias in one pass; ``y`` (optional): LN(x) itself"""
    check(lib.ltrx_norm_head_fwd(P(x), P(a), P(b), P(w), P(bias), rows, x.shape[-1], float(eps), P(scores), P(mean), P(rstd), P(y), st),
          "norm_head_fwd")


def norm_head_wgrad(lib, st, ds, xsum, a, b, mean, rstd, rows, dw, db, ws):
    """the head's own gradients from the recomputed LN(xsum), in ``score_head_bwd``'s row order"""
    check(lib.ltrx_norm_head_wgrad(P(ds), P(xsum), P(a), P(b), P(mean), P(rstd), rows, xsum.shape[-1], P(dw), P(db), P(ws), st),
          "norm_head_wgrad")


def norm_head_bwd_partial(lib, st, ds, xsum, a, w, mean, rstd, rows, eps, dx, ws):
    """dx of the fused pair now; returns how many rows of [da | db] partials the call left in ``ws`` for the caller to sum"""
    rows_out = ctypes.c_int(0)
    check(lib.ltrx_norm_head_bwd_partial(P(ds), P(xsum), P(a), P(w), P(mean), P(rstd), rows, xsum.shape[-1], float(eps), P(dx), P(ws),
                                         ctypes.byref(rows_out), st), "norm_head_bwd_partial")
    return rows_out.value


# ---- the optimizer over the flat buffers ----------------------------------------------------------------------------------
def clip_workspace(lib, n, like):
    return workspace(lib.ltrx_clip_workspace_bytes(n), like)


def clip_grad_norm_scale(lib, st, grads, max_norm, scale, norm, ws):
    """scale[0] = min(1, max_norm / (||grads|| + 1e-6)) -- what the optimizer launches take as ``grad_scale`` -- and norm[0] = the norm"""
    check(lib.ltrx_clip_grad_norm_scale(P(grads), grads.numel(), max_norm, P(scale), P(norm), P(ws), st), "clip_grad_norm")


def sgd_step(lib, st, params, grads, momentum_buf, lr, momentum, nesterov, weight_decay, grad_scale=None):
    """torch.optim.SGD over the flat buffers; ``momentum_buf`` None: no momentum; ``grad_scale``: the device float of the clip"""
    check(lib.ltrx_sgd_step(P(params), P(grads), P(momentum_buf), params.numel(), float(lr), momentum, 1 if nesterov else 0, weight_decay,
                            1.0, P(grad_scale), st), "sgd_step")


def adam_step(lib, st, params, grads, exp_avg, exp_avg_sq, lr, betas, eps, weight_decay, decoupled, step_count, grad_scale=None):
    """torch.optim.Adam (``decoupled``: AdamW) over the flat buffers; ``grad_scale``: the device float of the clip"""
    check(lib.ltrx_adam_step(P(params), P(grads), P(exp_avg), P(exp_avg_sq), params.numel(), float(lr), float(betas[0]), float(betas[1]),
                             float(eps), weight_decay, 1 if decoupled else 0, P(step_count), 1.0, P(grad_scale), st), "adam_step")


def first_nonfinite(lib, st, buf, seg_start, out):
    """out[0] = the first segment of ``buf`` (segment s starts at seg_start[s]) that holds a NaN / Inf, out[1] = how many elements do"""
    check(lib.ltrx_first_nonfinite(P(buf), buf.numel(), P(seg_start), seg_start.numel(), P(out), st), "first_nonfinite")


# ---- the slate-resident FC + ListNet step: forward, loss, backward and -- with ``opt`` -- Adam in two launches ----------------
def fc_listnet_workspace(lib, B, L, F, H, nflat, like):
    return workspace(lib.ltrx_fc_listnet_workspace_bytes(B, L, F, H, nflat), like)


def fc_linear_listnet_workspace(lib, B, F, like):
    return workspace(lib.ltrx_fc_linear_listnet_workspace_bytes(B, F), like)


_NO_OPT = (None, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, 0)


def fc_listnet_step(lib, st, x, y, B, L, H, act, params, off_w1, off_b1, off_wout, off_bout, eps, pad_value, divisor, scores, loss,
                    grads, ws, opt=None, hidden=None, dscores=None):
    """one step on the batch ``x`` [B * L, F], ``y`` [B, L] read in place: scores, the loss, the flat gradient.  ``opt`` = (exp_avg,
    exp_avg_sq, step_count, lr, beta1, beta2, eps, weight_decay, decoupled): the reducing launch also applies Adam; None: gradients
    only.  ``hidden`` / ``dscores`` (optional): the FC activation / d loss / d scores are written out too."""
    m, v, step, lr, b1, b2, aeps, wd, dec = opt or _NO_OPT
    check(lib.ltrx_fc_listnet_step(P(x), P(y), B, L, x.shape[-1], H, act, P(params), off_w1, off_b1, off_wout, off_bout, params.numel(),
                                   float(eps), float(pad_value), divisor, P(scores), P(dscores), P(hidden), P(loss), P(grads), P(m), P(v),
                                   P(step), lr, b1, b2, aeps, wd, dec, P(ws), st), "fc_listnet_step")


def fc_linear_listnet_step(lib, st, x, y, B, L, H, params, off_w1, off_b1, off_wout, off_bout, eps, pad_value, divisor, scores, loss,
                           grads, ws, opt=None, dscores=None):
    """the same step for a linear scorer (no FC activation, nothing hidden to write): one matrix-vector product per slate"""
    m, v, step, lr, b1, b2, aeps, wd, dec = opt or _NO_OPT
    check(lib.ltrx_fc_linear_listnet_step(P(x), P(y), B, L, x.shape[-1], H, P(params), off_w1, off_b1, off_wout, off_bout, params.numel(),
                                          float(eps), float(pad_value), divisor, P(scores), P(dscores), P(loss), P(grads), P(m), P(v),
                                          P(step), lr, b1, b2, aeps, wd, dec, P(ws), st), "fc_linear_listnet_step")


# ---- ranking and clicks on ragged slates (allrank_amd/inference.py, allrank_amd/clicks.py) -----------------------------------
def rank_slates_cu(lib, st, scores, cu, order, B, max_len, L, x_out, y_out, perm=None, x=None, y=None, slates=None, ids=None):
    """slates 0 .. B-1 of a ragged batch in ranked order into ``x_out`` [.., L, F] / ``y_out`` [.., L] (``perm``: the int32 order).
    Source rows: the padded grid ``x`` [.., L, F], ``y`` [.., L] -- or the resident set ``slates`` with the batch's device ``ids``."""
    res = slates is not None
    check(lib.ltrx_rank_slates_cu(P(scores), P(x), P(y), P(slates.x_items) if res else None, P(slates.y_items) if res else None,
                                  P(slates.offsets) if res else None, P(ids), P(cu), P(order), B, max_len, x_out.shape[-1], L, P(perm),
                                  P(x_out), P(y_out), st), "rank_slates_cu")


def click_slates_cu(lib, st, x, y, cu, order, B, max_len, clicks_out, plan, u=None, observe_p=None, margin_out=None, ws=None):
    """clicks of ``plan`` on slates 0 .. B-1 of the padded ranked batch ``x`` [B, L, F], ``y`` [B, L] into ``clicks_out`` [B, L]"""
    q = ctypes.c_double(plan["q"])
    check(lib.ltrx_click_slates_cu(P(x), P(y), P(cu), P(order), B, max_len, x.shape[-1], x.shape[-2], P(u), P(observe_p),
                                   float(plan["threshold"]), plan["max_candidates"], plan["diverse"],
                                   ctypes.c_void_p(ctypes.addressof(q)), plan["max_clicks"], P(clicks_out), P(margin_out), P(ws), st),
          "click_slates_cu")


# ---- the lane layout the attention kernels assume ---------------------------------------------------------------------------
def selftest_mfma32x32x2(lib, st, A, B, D):
    """D [32, 32] = A [32, 2] B [2, 32] through one MFMA"""
    check(lib.ltrx_selftest_mfma32x32x2(P(A), P(B), P(D), st), "selftest")
