"""Listwise losses and metrics on a RAGGED batch: only the valid items of every slate, one slate after the other, with the slate
extents in ``cu_seqlens`` -- the layout the attention kernels already take (include/ltrx.h, "Ragged layout").

    y_pred[n], y_true[n]     the valid items; slate b is rows cu_seqlens[b] .. cu_seqlens[b+1]-1
    cu_seqlens               int32 [B+1] on the device, cu_seqlens[0] = 0, n = cu_seqlens[B]; a slate may be empty
    max_len                  host int, an upper bound of every slate's length (it sizes the kernels' work arrays).  None: taken from
                             ``cu_seqlens`` -- ONE device-to-host sync; callers that know their lengths on the host pass it
    slate_order              int32 [B] on the device or None: the launch order of the slates (longest first balances the CUs);
                             results do not depend on it

Each function returns what its padded namesake (allrank_amd.losses / allrank_amd.metrics) returns on the [B, L] grid that holds
every slate's items first and the padding value after them, for any L >= max_len: the same kernel bodies run, with their loops
bounded by the slate's own length instead of L.  The keyword arguments are the namesake's without ``padded_value_indicator`` /
``padding_indicator`` -- no row is padding.  The losses are differentiable the same way (the fused kernel leaves d loss / d y_pred,
the autograd node scales it) and go through the same plugin call, so ``sharding.shard_context`` divisors and lambdaLoss's
batch-global pair count work as they do there.  Device tensors only.

``form_of(loss_func)`` maps a padded loss (or a functools.partial of one) to its ragged form, None where there is none.
"""
import ctypes
import functools

import torch

from . import _lib as L
from . import losses as E
from . import metrics as EM

DEFAULT_EPS = E.DEFAULT_EPS

__all__ = ["listNet", "approxNDCGLoss", "lambdaLoss", "ndcg", "dcg", "mrr", "form_of"]


def _layout(y_pred, y_true, cu_seqlens, max_len, slate_order):
    """checks of the layout arguments; (cu int32 contiguous, order or None, B, max_len as a host int)"""
    L.require_device(y_pred, y_true, cu_seqlens, slate_order)
    if cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 or cu_seqlens.dtype != torch.int32:
        raise ValueError("cu_seqlens must be an int32 tensor [number of slates + 1]")
    cu = cu_seqlens.contiguous()
    B = int(cu.numel()) - 1
    order = None
    if slate_order is not None:
        if slate_order.dtype != torch.int32 or slate_order.numel() != B:
            raise ValueError("slate_order must be an int32 tensor [number of slates]")
        order = slate_order.contiguous()
    if max_len is None:
        max_len = int((cu[1:] - cu[:-1]).max().item())          # (the documented host sync)
    return cu, order, B, max(int(max_len), 1)                   # (a batch of empty slates still launches: work arrays of one item)


# ----------------------------------------------------------------------------------------------------------------
# launchers of the *_cu entry points, in the form losses._call takes them (losses._Family): ``a`` carries the bound arguments,
# ``cu`` / ``order`` arrive as the call's extra buffers, the shape (B, max_len) through _call's ``shape``
# ----------------------------------------------------------------------------------------------------------------
def _launch_listnet(yp, yt, a, div, loss, grad, ws, cu, order):
    L.check(L.lib().ltrx_listnet_fwd_bwd_cu(L.ptr(yp), L.ptr(yt), L.ptr(cu), L.ptr(order), cu.numel() - 1, a["max_len"], float(a["eps"]),
                                            div, L.ptr(loss), None, L.ptr(grad), L.ptr(ws), L.stream_of(yp)), "listnet_cu")


def _launch_approxndcg(yp, yt, a, div, loss, grad, ws, cu, order):
    L.check(L.lib().ltrx_approxndcg_fwd_bwd_cu(L.ptr(yp), L.ptr(yt), L.ptr(cu), L.ptr(order), cu.numel() - 1, a["max_len"],
                                               float(a["eps"]), float(a["alpha"]), div, L.ptr(loss), None, L.ptr(grad), L.ptr(ws),
                                               L.stream_of(yp)), "approxndcg_cu")


def _launch_lambdaloss(yp, yt, a, div, loss, grad, ws, cnt, cu, order):
    red = 0 if a["reduction"] == "sum" else 1
    lg = 0 if a["reduction_log"] == "binary" else 1

    def call(ext, cnt, grad):       # (the count pass: a 'sum' pass that also writes the pair count)
        return L.lib().ltrx_lambdaloss_fwd_bwd_cu(L.ptr(yp), L.ptr(yt), L.ptr(cu), L.ptr(order), cu.numel() - 1, a["max_len"],
                                                  float(a["eps"]), E._SCHEMES[a["weighing_scheme"]], 0 if a["k"] is None else int(a["k"]),
                                                  float(a["sigma"]), float(a["mu"]), 0 if cnt is not None else red, lg, L.ptr(ext),
                                                  L.ptr(loss), L.ptr(cnt), L.ptr(grad), None, L.ptr(ws), L.stream_of(yp))
    E._count_normalised(call, cnt, grad, "lambdaloss_cu", sharded=red == 1)


_LISTNET = E._Family(_launch_listnet, E._LISTNET.ws_bytes, ())
_APPROXNDCG = E._Family(_launch_approxndcg, E._APPROXNDCG.ws_bytes, ())
_LAMBDALOSS = E._Family(_launch_lambdaloss, E._LAMBDALOSS.ws_bytes, ("cnt",))


def _call(fam, y_pred, y_true, cu_seqlens, max_len, slate_order, a):
    cu, order, B, max_len = _layout(y_pred, y_true, cu_seqlens, max_len, slate_order)
    return E._call(fam, y_pred, y_true, dict(a, max_len=max_len), shape=(B, max_len), cu=cu, order=order)


def listNet(y_pred, y_true, cu_seqlens, max_len=None, slate_order=None, eps=DEFAULT_EPS):
    """``losses.listNet`` on a ragged batch; an empty slate contributes 0."""
    return _call(_LISTNET, y_pred, y_true, cu_seqlens, max_len, slate_order, dict(eps=eps))


def approxNDCGLoss(y_pred, y_true, cu_seqlens, max_len=None, slate_order=None, eps=DEFAULT_EPS, alpha=1.):
    """``losses.approxNDCGLoss`` on a ragged batch; an empty slate contributes 0."""
    return _call(_APPROXNDCG, y_pred, y_true, cu_seqlens, max_len, slate_order, dict(eps=eps, alpha=alpha))


def lambdaLoss(y_pred, y_true, cu_seqlens, max_len=None, slate_order=None, eps=DEFAULT_EPS, weighing_scheme=None, k=None, sigma=1.,
               mu=10., reduction="sum", reduction_log="binary"):
    """``losses.lambdaLoss`` on a ragged batch (all weighing schemes; 'mean' divides by the batch-global pair count)."""
    a = dict(eps=eps, weighing_scheme=weighing_scheme, k=k, sigma=sigma, mu=mu, reduction=reduction, reduction_log=reduction_log)
    E._check_lambdaloss(a)
    return _call(_LAMBDALOSS, y_pred, y_true, cu_seqlens, max_len, slate_order, a)


# ----------------------------------------------------------------------------------------------------------------
# metrics
# ----------------------------------------------------------------------------------------------------------------
def _metric_inputs(y_pred, y_true, cu_seqlens, max_len, slate_order, ats):
    if y_pred.dim() != 1 or y_pred.shape != y_true.shape:
        raise ValueError("y_pred and y_true must both be [n], the valid items of the batch's slates one after the other")
    cu, order, B, max_len = _layout(y_pred, y_true, cu_seqlens, max_len, slate_order)
    ats = [max_len] if ats is None else [int(a) for a in ats]          # metrics.py:58-59; a cut-off above a slate's length is its length
    return L.f32c(y_pred.detach()), L.f32c(y_true.detach()), cu, order, B, max_len, ats, (ctypes.c_int * len(ats))(*ats)


def _ndcg(y_pred, y_true, cu_seqlens, max_len, slate_order, ats, gain_function, filler_value, want_order):
    if gain_function is not None:
        raise ValueError("allrank_amd.ragged: a custom gain_function has no ragged form (use allrank_amd.metrics on the padded grid)")
    yp, yt, cu, order, B, max_len, ats, arr = _metric_inputs(y_pred, y_true, cu_seqlens, max_len, slate_order, ats)
    nd = torch.empty((B, len(ats)), dtype=torch.float32, device=yp.device)
    dc = torch.empty((B, len(ats)), dtype=torch.float32, device=yp.device)
    perm = torch.empty(yp.shape, dtype=torch.int64, device=yp.device) if want_order else None
    L.check(L.lib().ltrx_ndcg_at_cu(L.ptr(yp), L.ptr(yt), L.ptr(cu), L.ptr(order), B, max_len, arr, len(ats), float(filler_value),
                                    L.ptr(nd), L.ptr(dc), L.ptr(perm), None, L.stream_of(yp)), "ndcg_at_cu")
    return nd, dc, perm


def ndcg(y_pred, y_true, cu_seqlens, max_len=None, slate_order=None, ats=None, gain_function=None, filler_value=1.0,
         return_order=False):
    """``metrics.ndcg`` on a ragged batch: [B, len(ats)]; slates without a relevant item -- empty ones included -- get
    ``filler_value``.  ``return_order``: also the stable descending argsort [n], as indices inside each slate."""
    nd, _, perm = _ndcg(y_pred, y_true, cu_seqlens, max_len, slate_order, ats, gain_function, filler_value, return_order)
    return (nd, perm) if return_order else nd


def dcg(y_pred, y_true, cu_seqlens, max_len=None, slate_order=None, ats=None, gain_function=None):
    """``metrics.dcg`` on a ragged batch: [B, len(ats)], 0 for an empty slate."""
    return _ndcg(y_pred, y_true, cu_seqlens, max_len, slate_order, ats, gain_function, 1.0, False)[1]


def mrr(y_pred, y_true, cu_seqlens, max_len=None, slate_order=None, ats=None):
    """``metrics.mrr`` on a ragged batch: [B, len(ats)], with the reference's batch-level zeroing (all maxima 0)."""
    yp, yt, cu, order, B, max_len, ats, arr = _metric_inputs(y_pred, y_true, cu_seqlens, max_len, slate_order, ats)
    out = torch.empty((B, len(ats)), dtype=torch.float32, device=yp.device)
    lib = L.lib()
    ws = L.workspace(lib.ltrx_mrr_workspace_bytes(B, max_len, len(ats)), yp)
    L.check(lib.ltrx_mrr_at_cu(L.ptr(yp), L.ptr(yt), L.ptr(cu), L.ptr(order), B, max_len, arr, len(ats), L.ptr(out), L.ptr(ws),
                               L.stream_of(yp)), "mrr_at_cu")
    return out


# ----------------------------------------------------------------------------------------------------------------
# padded callable -> ragged callable
# ----------------------------------------------------------------------------------------------------------------
_FORMS = {E.listNet: listNet, E.approxNDCGLoss: approxNDCGLoss, E.lambdaLoss: lambdaLoss, EM.ndcg: ndcg, EM.dcg: dcg, EM.mrr: mrr}
_PAD_ARGS = ("padded_value_indicator", "padding_indicator")


def form_of(loss_func):
    """The ragged form of a padded loss of ``allrank_amd.losses`` (or metric of ``allrank_amd.metrics``), given as the function
    itself or as a ``functools.partial`` of it: the ragged callable with the same bound keyword arguments -- minus the padding
    value, which the layout does not have.  None where there is no ragged form: listMLE (its ``perm`` shuffles padded columns),
    the NeuralNDCG losses, the pointwise and pairwise losses, a metric bound to a custom ``gain_function``, positionally bound
    arguments, and anything that is not one of this package's functions."""
    func, kw = loss_func, {}
    if isinstance(loss_func, functools.partial):
        if loss_func.args:
            return None
        func, kw = loss_func.func, dict(loss_func.keywords or {})
    try:
        rag = _FORMS.get(func)
    except TypeError:                       # (an unhashable callable)
        return None
    if rag is None or kw.get("gain_function") is not None:
        return None
    kw = {k: v for k, v in kw.items() if k not in _PAD_ARGS}
    return functools.partial(rag, **kw) if kw else rag
