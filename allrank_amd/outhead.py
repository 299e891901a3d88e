"""The two kernel calls that serve a model with several output units (OutputLayer(d, d_output > 1): the ordinal configurations) on the
forward-only scorer and in the ranking, stated once, in the form of allrank_amd/kernels.py: one ``ltrx_*`` call on the tensors handed
in, the bound library ``lib`` and the stream ``st`` as arguments, nothing allocated, no device checked.  allrank_amd/kernels.py hands
both names on, so the engine and allrank_amd/inference.py launch them as they launch every other kernel.

  ``out_head_fwd``         include/ltrx.h, ltrx_out_head_fwd (allrank_amd/csrc/ltrx_outhead.hip): Linear + activation + the sum over
                           the output units, one launch, exact fp32.
  ``rank_slates_rows_cu``  include/ltrx.h, ltrx_rank_slates_rows_cu (allrank_amd/csrc/ltrx_rank.hip): ``rank_slates_cu`` with the sort
                           key formed from the packed output rows.
"""
from ._lib import check, ptr as P

UNSUPPORTED = -2                                             # LTRX_EUNSUPPORTED


def out_head_fwd(lib, st, x, w, bias, rows, act, out=None, score=None):
    """out[:rows] = act(x[:rows] w^T + bias) ([rows, n_out], dense) and score[:rows] = its sum over the output units; ``x`` may be a
    column slice of a wider buffer (its row stride is read from it), ``w`` is the module's [n_out, D] weight.  Returns False -- and
    has launched nothing -- where the library does not take the shape (the caller keeps its GEMM sequence); any other refusal raises."""
    rc = lib.ltrx_out_head_fwd(P(x), x.stride(0), P(w), P(bias), rows, x.shape[1], w.shape[0], act, P(out), P(score), st)
    if rc != UNSUPPORTED:
        check(rc, "out_head_fwd")
    return rc != UNSUPPORTED


def rank_slates_rows_cu(lib, st, out, cu, order, B, max_len, L, x_out, y_out, perm=None, x=None, y=None, slates=None, ids=None):
    """``kernels.rank_slates_cu`` for the packed output rows ``out`` [n, n_out] of a model with several output units: an item's sort key
    is the sum of its row, formed in the kernel"""
    res = slates is not None
    check(lib.ltrx_rank_slates_rows_cu(P(out), out.shape[1], P(x), P(y), P(slates.x_items) if res else None,
                                       P(slates.y_items) if res else None, P(slates.offsets) if res else None, P(ids), P(cu), P(order), B,
                                       max_len, x_out.shape[-1], L, P(perm), P(x_out), P(y_out), st), "rank_slates_rows_cu")
