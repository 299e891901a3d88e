"""MI355X-native listwise losses with the plugin signatures of ``allrank.models.losses``.

Every function here has the signature, defaults, error behaviour and semantics of its namesake in the reference
(allrank/models/losses/__init__.py:3-12; selected by name at allrank/main.py:83) and returns a 0-dim tensor that
supports ``.backward()`` / ``.item()``.  The arithmetic runs in ONE fused HIP kernel per loss (forward and
d loss / d y_pred together; libltrx.so, include/ltrx.h); the autograd node only scales the stored gradient.
Inputs are never mutated.  Device tensors only -- there is no CPU fallback.
"""
import collections
import contextlib
import inspect
import threading

import torch

from .. import _lib as L
from .. import sharding

DEFAULT_EPS = 1e-10        # allrank/models/losses/__init__.py:1
PADDED_Y_VALUE = -1        # allrank/data/dataset_loading.py:15

__all__ = ["DEFAULT_EPS", "PADDED_Y_VALUE", "listNet", "listMLE", "approxNDCGLoss", "lambdaLoss", "neuralNDCG",
           "neuralNDCG_transposed", "sinkhorn_iterations_used", "rankNet", "rankNet_weightByGTDiff",
           "rankNet_weightByGTDiff_pow", "bce", "ordinal", "with_ordinals", "pointwise_rmse", "binary_listNet"]

_SCHEMES = {None: 0, "ndcgLoss1_scheme": 1, "ndcgLoss2_scheme": 2, "lambdaRank_scheme": 3, "ndcgLoss2PP_scheme": 4,
            "rankNet_scheme": 5, "rankNetWeightedByGTDiff_scheme": 6, "rankNetWeightedByGTDiffPowed_scheme": 7}


class _FusedLoss(torch.autograd.Function):
    """The kernel already produced d loss / d y_pred; backward is a scale by the incoming gradient."""

    @staticmethod
    def forward(ctx, y_pred, loss, grad):
        ctx.save_for_backward(grad)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def _prep(y_pred, y_true, n=None, ragged=False):
    """shape and device checks; (float32 contiguous scores, labels, whether a gradient is wanted).  ``n``: ordinal's [B, L, n] scores;
    ``ragged``: the [n] tensors of the cu_seqlens layout (allrank_amd.ragged)"""
    if ragged and (y_pred.dim() != 1 or y_pred.shape != y_true.shape):
        raise ValueError("y_pred and y_true must both be [n], the valid items of the batch's slates one after the other")
    if n is None and not ragged and (y_pred.dim() != 2 or y_pred.shape != y_true.shape):
        raise ValueError("y_pred and y_true must both be [batch_size, slate_length]")
    if n is not None and (y_pred.dim() != 3 or y_pred.shape[:2] != y_true.shape or y_pred.shape[2] != n):
        raise ValueError("y_pred must be [batch_size, slate_length, n] and y_true [batch_size, slate_length]")
    L.require_device(y_pred, y_true)
    return L.f32c(y_pred.detach()), L.f32c(y_true.detach()), torch.is_grad_enabled() and y_pred.requires_grad


def _finish(y_pred, loss, grad, need_grad):
    if need_grad:
        return _FusedLoss.apply(y_pred, loss, grad.to(y_pred.dtype))
    return loss.view(())


# ----------------------------------------------------------------------------------------------------------------
# One launcher per kernel family: ``launch(yp, yt, a, div, loss, grad, ws, ...)`` makes the family's ltrx_* call(s) on the buffers it
# is handed -- fresh ones from a plugin call (_call), persistent ones from FusedLoss -- with ``a`` the loss's fully bound arguments,
# ``div`` the batch divisor, ``grad`` None for a loss-only pass, and the ``extra`` buffers by keyword.
# ----------------------------------------------------------------------------------------------------------------
_Family = collections.namedtuple("_Family", "launch ws_bytes extra")     # ws_bytes(B, SL, a); extra: of "cnt" [1], "idcg" [B]


def _buffers(fam, B, SL, device, a, new):
    """loss[1], the family's workspace and extra buffers for B slates of SL items; ``new`` = torch.empty or torch.zeros"""
    bufs = {k: new(B if k == "idcg" else 1, dtype=torch.float32, device=device) for k in ("loss",) + fam.extra}
    bufs["ws"] = torch.empty(max(int(fam.ws_bytes(B, SL, a)), 64), dtype=torch.uint8, device=device)
    return bufs


def _call(fam, y_pred, y_true, a, n=None, shape=None, **given):
    """a plugin call: fresh buffers (plus the ``given`` ones), the family's launcher, the autograd node.  ``shape``: (slates, max_len)
    of a call in the cu_seqlens layout (allrank_amd.ragged), whose tensors are [n] and do not carry it"""
    yp, yt, need_grad = _prep(y_pred, y_true, n, ragged=shape is not None)
    B, SL = shape if shape is not None else yt.shape
    bufs = dict(_buffers(fam, B, SL, yp.device, a, torch.empty), **given)
    grad = torch.empty_like(yp) if need_grad else None
    fam.launch(yp, yt, a, sharding.batch_divisor(B), grad=grad, **bufs)
    return _finish(y_pred, bufs["loss"], grad, need_grad)


def _count_normalised(call, cnt, grad, what, sharded=True):
    """the losses whose divisor is a batch-global count, ``call(ext, cnt, grad)`` -> status: under slate sharding a loss-only pass
    produces this rank's count, the counts are all-reduced, and the real pass divides by the global one"""
    ext = None
    if sharded and sharding.active():
        L.check(call(None, cnt, None), what + "(count)")
        ext = sharding.allreduce_sum_(cnt)
    L.check(call(ext, None, grad), what)


def _launch_listnet(yp, yt, a, div, loss, grad, ws):
    B, SL = yt.shape
    L.check(L.lib().ltrx_listnet_fwd_bwd(L.ptr(yp), L.ptr(yt), B, SL, float(a["eps"]), float(a["padded_value_indicator"]), div,
                                         L.ptr(loss), None, L.ptr(grad), L.ptr(ws), L.stream_of(yp)), "listnet")


def _launch_listmle(yp, yt, a, div, loss, grad, ws, perm):
    B, SL = yt.shape
    L.check(L.lib().ltrx_listmle_fwd_bwd(L.ptr(yp), L.ptr(yt), L.ptr(perm), B, SL, float(a["eps"]), float(a["padded_value_indicator"]),
                                         div, L.ptr(loss), None, L.ptr(grad), None, L.ptr(ws), L.stream_of(yp)), "listmle")


def _launch_approxndcg(yp, yt, a, div, loss, grad, ws):
    B, SL = yt.shape
    L.check(L.lib().ltrx_approxndcg_fwd_bwd(L.ptr(yp), L.ptr(yt), B, SL, float(a["eps"]), float(a["padded_value_indicator"]),
                                            float(a["alpha"]), div, L.ptr(loss), None, L.ptr(grad), L.ptr(ws), L.stream_of(yp)),
            "approxndcg")


def _check_lambdaloss(a):
    if a["weighing_scheme"] not in _SCHEMES:
        raise KeyError(a["weighing_scheme"])                             # reference: globals()[weighing_scheme] (:61)
    if a["reduction_log"] not in ("natural", "binary"):
        raise ValueError("Reduction logarithm base can be either natural or binary")   # lambdaLoss.py:72
    if a["reduction"] not in ("sum", "mean"):
        raise ValueError("Reduction method can be either sum or mean")                  # lambdaLoss.py:79


def _launch_lambdaloss(yp, yt, a, div, loss, grad, ws, cnt):
    B, SL = yt.shape
    red = 0 if a["reduction"] == "sum" else 1
    lg = 0 if a["reduction_log"] == "binary" else 1

    def call(ext, cnt, grad):       # (the count pass: a 'sum' pass that also writes the pair count)
        return L.lib().ltrx_lambdaloss_fwd_bwd(L.ptr(yp), L.ptr(yt), B, SL, float(a["eps"]), float(a["padded_value_indicator"]),
                                               _SCHEMES[a["weighing_scheme"]], 0 if a["k"] is None else int(a["k"]), float(a["sigma"]),
                                               float(a["mu"]), 0 if cnt is not None else red, lg, L.ptr(ext), L.ptr(loss), L.ptr(cnt),
                                               L.ptr(grad), None, L.ptr(ws), L.stream_of(yp))
    _count_normalised(call, cnt, grad, "lambdaloss", sharded=red == 1)


def _neural_prepare(yt, a, idcg, cnt, ws):
    """per-slate ideal DCG and the batch-global normaliser (neuralNDCG.py:69) of the slates ``yt``"""
    B, SL = yt.shape
    idcg_powered = 1 if (a["powered_relevancies"] or a["transposed"]) else 0       # neuralNDCG.py:55-58 vs :118-126
    L.check(L.lib().ltrx_neuralndcg_prepare(L.ptr(yt), B, SL, float(a["padded_value_indicator"]), 0 if a["k"] is None else int(a["k"]),
                                            idcg_powered, L.ptr(idcg), L.ptr(cnt), L.ptr(ws), L.stream_of(yt)), "neuralndcg_prepare")
    sharding.allreduce_sum_(cnt)


def _launch_neuralndcg(yp, yt, a, div, loss, grad, ws, idcg, cnt, iters=None, k_rows=None, prepared=False):
    """fused NeuralSort + Sinkhorn + value + gradient; ``prepared``: idcg / cnt are already filled (the stochastic form, whose
    pseudo slates carry the idcg of their source slate, ranks beyond ``k_rows`` without discount)"""
    B, SL = yt.shape
    if not prepared:
        _neural_prepare(yt, a, idcg, cnt, ws)
    L.check(L.lib().ltrx_neuralndcg_fwd_bwd(L.ptr(yp), L.ptr(yt), L.ptr(idcg), L.ptr(cnt), B, SL, float(a["padded_value_indicator"]),
                                            float(a["temperature"]), 1 if a["powered_relevancies"] else 0,
                                            0 if a["k"] is None else int(a["k"]), L.ptr(k_rows), 1 if a["transposed"] else 0,
                                            int(a["max_iter"]), float(a["tol"]), L.ptr(loss), None, L.ptr(grad), L.ptr(iters),
                                            _neural_path(), L.ptr(ws), L.stream_of(yp)), "neuralndcg")
    if iters is not None:
        _last_iters["t"] = iters


def _launch_ranknet(yp, yt, a, div, loss, grad, ws, cnt):
    B, SL = yt.shape
    mode = 1 if a["weight_by_diff"] else (2 if a["weight_by_diff_powed"] else 0)           # rankNet.py:63-70 (elif order)

    def call(ext, cnt, grad):
        return L.lib().ltrx_ranknet_fwd_bwd(L.ptr(yp), L.ptr(yt), B, SL, float(a["padded_value_indicator"]), mode, L.ptr(ext),
                                            L.ptr(loss), L.ptr(cnt), L.ptr(grad), L.ptr(ws), L.stream_of(yp))
    _count_normalised(call, cnt, grad, "ranknet")


def _launch_bce(yp, yt, a, div, loss, grad, ws, cnt):
    """bce: scores [B, SL] probabilities, n = 0; ordinal: scores [B, SL, n] (n = the OutputLayer's d_output, ordinal.py:25-50)"""
    B, SL = yt.shape

    def call(ext, cnt, grad):
        return L.lib().ltrx_bce_fwd_bwd(L.ptr(yp), L.ptr(yt), B, SL, int(a["n"]), float(a["padded_value_indicator"]), L.ptr(ext),
                                        L.ptr(loss), L.ptr(cnt), L.ptr(grad), L.ptr(ws), L.stream_of(yp))
    _count_normalised(call, cnt, grad, "ordinal" if a["n"] else "bce")


def _launch_pointwise_rmse(yp, yt, a, div, loss, grad, ws):
    B, SL = yt.shape
    L.check(L.lib().ltrx_pointwise_rmse_fwd_bwd(L.ptr(yp), L.ptr(yt), B, SL, float(a["no_of_levels"]), float(a["padded_value_indicator"]),
                                                div, L.ptr(loss), L.ptr(grad), L.ptr(ws), L.stream_of(yp)), "pointwise_rmse")


def _launch_binary_listnet(yp, yt, a, div, loss, grad, ws):
    B, SL = yt.shape
    L.check(L.lib().ltrx_binary_listnet_fwd_bwd(L.ptr(yp), L.ptr(yt), B, SL, float(a["eps"]), float(a["padded_value_indicator"]), div,
                                                L.ptr(loss), L.ptr(grad), L.ptr(ws), L.stream_of(yp)), "binary_listnet")


_LISTNET = _Family(_launch_listnet, lambda B, SL, a: L.lib().ltrx_listnet_workspace_bytes(B, SL), ())
_LISTMLE = _Family(_launch_listmle, lambda B, SL, a: L.lib().ltrx_listmle_workspace_bytes(B, SL), ())
_APPROXNDCG = _Family(_launch_approxndcg, lambda B, SL, a: L.lib().ltrx_approxndcg_workspace_bytes(B, SL), ())
_LAMBDALOSS = _Family(_launch_lambdaloss, lambda B, SL, a: L.lib().ltrx_lambdaloss_workspace_bytes(B, SL), ("cnt",))
_NEURALNDCG = _Family(_launch_neuralndcg, lambda B, SL, a: L.lib().ltrx_neuralndcg_workspace_bytes(B, SL, int(a["max_iter"])),
                      ("idcg", "cnt"))
_RANKNET = _Family(_launch_ranknet, lambda B, SL, a: L.lib().ltrx_ranknet_workspace_bytes(B, SL), ("cnt",))
_BCE = _Family(_launch_bce, lambda B, SL, a: L.lib().ltrx_bce_workspace_bytes(B, SL, int(a["n"])), ("cnt",))
_POINTWISE_RMSE = _Family(_launch_pointwise_rmse, lambda B, SL, a: L.lib().ltrx_pointwise_rmse_workspace_bytes(B, SL), ())
_BINARY_LISTNET = _Family(_launch_binary_listnet, lambda B, SL, a: L.lib().ltrx_binary_listnet_workspace_bytes(B, SL), ())

# loss name -> (family, the arguments the name itself fixes: what its plugin function passes on beyond its own signature)
_LOSSES = {"listNet": (_LISTNET, {}), "listMLE": (_LISTMLE, {}), "approxNDCGLoss": (_APPROXNDCG, {}), "lambdaLoss": (_LAMBDALOSS, {}),
           "neuralNDCG": (_NEURALNDCG, dict(transposed=False, max_iter=50, tol=1e-6)),        # Sinkhorn: neuralNDCG.py:10-70
           "neuralNDCG_transposed": (_NEURALNDCG, dict(transposed=True)),
           "rankNet": (_RANKNET, {}), "rankNet_weightByGTDiff": (_RANKNET, dict(weight_by_diff=True, weight_by_diff_powed=False)),
           "rankNet_weightByGTDiff_pow": (_RANKNET, dict(weight_by_diff=False, weight_by_diff_powed=True)),
           "bce": (_BCE, dict(n=0)), "ordinal": (_BCE, {}), "pointwise_rmse": (_POINTWISE_RMSE, {}),
           "binary_listNet": (_BINARY_LISTNET, {})}


# ----------------------------------------------------------------------------------------------------------------
# the plugin functions
# ----------------------------------------------------------------------------------------------------------------
def listNet(y_pred, y_true, eps=DEFAULT_EPS, padded_value_indicator=PADDED_Y_VALUE):
    """ListNet (allrank/models/losses/listNet.py:8-30): -mean_b sum_i softmax(y_true)_i log(softmax(y_pred)_i + eps)."""
    return _call(_LISTNET, y_pred, y_true, dict(eps=eps, padded_value_indicator=padded_value_indicator))


def listMLE(y_pred, y_true, eps=DEFAULT_EPS, padded_value_indicator=PADDED_Y_VALUE, perm=None, generator=None):
    """ListMLE (allrank/models/losses/listMLE.py:7-38).  The reference shuffles the columns with
    ``torch.randperm(L)`` from the global CPU generator (listMLE.py:17) for randomised tie resolution; so does this
    function unless ``perm`` (an int64 permutation of range(L), any device) is given.  Ties among equal labels are
    then resolved by a STABLE sort in the shuffled order."""
    if perm is None:
        perm = torch.randperm(y_true.shape[-1], generator=generator)     # CPU generator, like the reference
    perm = perm.to(device=y_pred.device, dtype=torch.int64).contiguous()
    if perm.numel() != y_true.shape[-1]:
        raise ValueError("perm must be a permutation of range(slate_length)")
    return _call(_LISTMLE, y_pred, y_true, dict(eps=eps, padded_value_indicator=padded_value_indicator), perm=perm)


def approxNDCGLoss(y_pred, y_true, eps=DEFAULT_EPS, padded_value_indicator=PADDED_Y_VALUE, alpha=1.):
    """ApproxNDCG (allrank/models/losses/approxNDCG.py:7-53); no truncation, sigmoid temperature ``alpha``."""
    return _call(_APPROXNDCG, y_pred, y_true, dict(eps=eps, padded_value_indicator=padded_value_indicator, alpha=alpha))


def lambdaLoss(y_pred, y_true, eps=DEFAULT_EPS, padded_value_indicator=PADDED_Y_VALUE, weighing_scheme=None, k=None,
               sigma=1., mu=10., reduction="sum", reduction_log="binary"):
    """LambdaLoss framework (allrank/models/losses/lambdaLoss.py:7-114) with its 7 weighing schemes."""
    a = dict(eps=eps, padded_value_indicator=padded_value_indicator, weighing_scheme=weighing_scheme, k=k, sigma=sigma, mu=mu,
             reduction=reduction, reduction_log=reduction_log)
    _check_lambdaloss(a)
    return _call(_LAMBDALOSS, y_pred, y_true, a)


_last_iters = {"t": None}
_neural_tls = threading.local()


@contextlib.contextmanager
def neural_kernel_path(path):
    """test hook (thread-local, scoped): 1 = run the general L2-streaming Sinkhorn kernels even where the register-resident
    ones apply (L <= 240); the value is passed as the ``path`` argument of every ltrx_neuralndcg_fwd_bwd call in the region."""
    prev = getattr(_neural_tls, "path", 0)
    _neural_tls.path = int(path)
    try:
        yield
    finally:
        _neural_tls.path = prev


def _neural_path():
    return getattr(_neural_tls, "path", 0)


def sinkhorn_iterations_used():
    """number of Sinkhorn iterations the last neuralNDCG* call ran (device->host sync; diagnostics only)."""
    t = _last_iters["t"]
    return None if t is None else int(t.item())


def sample_gumbel(samples_shape, device, eps=1e-10):
    """loss_utils.py:70-81"""
    U = torch.rand(samples_shape, device=device)
    return -torch.log(-torch.log(U + eps) + eps)


def _neural(y_pred, y_true, a, stochastic, n_samples, beta, log_scores, gumbel):
    """``a``: the bound arguments of the neuralndcg family (padded_value_indicator, temperature, powered_relevancies, k, transposed,
    max_iter, tol)"""
    if not stochastic:
        return _call(_NEURALNDCG, y_pred, y_true, a, iters=torch.empty(1, dtype=torch.int32, device=y_pred.device))
    yp, yt, _ = _prep(y_pred, y_true)
    B, SL = yt.shape
    pre = _buffers(_NEURALNDCG, B, SL, yp.device, a, torch.empty)
    _neural_prepare(yt, a, pre["idcg"], pre["cnt"], pre["ws"])
    # ---- stochastic NeuralSort (loss_utils.py:84-112): n_samples Gumbel-perturbed copies of every slate ----
    # The perturbation is a handful of elementwise torch ops (autograd carries d s_perturb / d y_pred, including the path
    # through the batch-global min); the n_samples * B perturbed slates then go through the SAME fused kernels as one batch.
    S = int(n_samples)
    s = y_pred.to(torch.float32)
    s_pos = s + torch.abs(s.min())                                       # :102 (min over the whole batch, padded slots too)
    if gumbel is None:
        gumbel = sample_gumbel([S, B, SL, 1], device=yp.device)          # :103
    samples = float(beta) * gumbel.to(device=yp.device, dtype=torch.float32).reshape(S, B, SL)
    if log_scores:
        s_pos = torch.log(s_pos + 1e-10)                                 # :104-105
    s_pert = (s_pos.unsqueeze(0) + samples).reshape(S * B, SL)           # pseudo slate i = sample i // B of slate i % B
    # The reference sorts pseudo slate i under the padding mask of slate i // n_samples (mask.repeat_interleave, :108 and
    # neuralNDCG.py:41/:106) but reads the result out with the labels of slate i % B.  Reproduced exactly through the labels
    # handed to the kernel:
    #   plain (:44-51: rows and columns are masked by the TRUE slate's padding, padded gains are 0):
    #     padding where the sort mask pads; the true label where both are valid; label 0 (= gain 0) where only the sort
    #     mask is valid; ranks beyond the true slate's length carry no discount (k_rows).
    #   transposed (:116-124: no read-out mask, gains are the RAW labels, i.e. 2^-1 - 1 or -1 on truly padded items):
    #     the raw labels wherever the sort mask is valid, under a private padding sentinel.
    idx = torch.arange(S * B, device=yp.device)
    sort_src, true_src = idx // S, idx % B
    pad = float(a["padded_value_indicator"])
    sort_pad = (yt[sort_src] == pad)
    true_pad = (yt[true_src] == pad)
    if a["transposed"]:
        pad_k = -1.0e30
        y_ps = torch.where(sort_pad, torch.full((), pad_k, device=yp.device), yt[true_src]).contiguous()
        k_rows = None
    else:
        pad_k = pad
        y_ps = torch.where(true_pad, torch.zeros((), device=yp.device), yt[true_src])
        y_ps = torch.where(sort_pad, torch.full((), pad, device=yp.device), y_ps).contiguous()
        k_rows = (~true_pad).sum(1).to(torch.int32).contiguous()
    sp = s_pert.detach().contiguous()
    ng = torch.is_grad_enabled() and s_pert.requires_grad
    a = dict(a, padded_value_indicator=pad_k)
    bufs = _buffers(_NEURALNDCG, S * B, SL, yp.device, a, torch.empty)
    bufs.update(idcg=pre["idcg"][true_src].contiguous(), cnt=pre["cnt"] * float(S))     # neuralNDCG.py:69: (#idcg != 0) * n_samples
    grad = torch.empty_like(sp) if ng else None
    _launch_neuralndcg(sp, y_ps, a, sharding.batch_divisor(S * B), grad=grad, k_rows=k_rows, prepared=True,
                       iters=torch.empty(1, dtype=torch.int32, device=yp.device), **bufs)
    return _finish(s_pert, bufs["loss"], grad, ng)


def neuralNDCG(y_pred, y_true, padded_value_indicator=PADDED_Y_VALUE, temperature=1., powered_relevancies=True, k=None,
               stochastic=False, n_samples=32, beta=0.1, log_scores=True, gumbel=None):
    """NeuralNDCG (allrank/models/losses/neuralNDCG.py:10-70): NeuralSort (deterministic, or stochastic with ``n_samples``
    Gumbel-perturbed copies per slate) + Sinkhorn (50 its, tol 1e-6).  ``gumbel`` ([n_samples, B, L, 1], optional) injects
    the Gumbel noise the reference draws with torch.rand (loss_utils.py:80) -- parity tests pass the same draw to both."""
    a = dict(padded_value_indicator=padded_value_indicator, temperature=temperature, powered_relevancies=powered_relevancies, k=k,
             **_LOSSES["neuralNDCG"][1])
    return _neural(y_pred, y_true, a, stochastic, n_samples, beta, log_scores, gumbel)


def neuralNDCG_transposed(y_pred, y_true, padded_value_indicator=PADDED_Y_VALUE, temperature=1.,
                          powered_relevancies=True, k=None, stochastic=False, n_samples=32, beta=0.1, log_scores=True,
                          max_iter=50, tol=1e-6, gumbel=None):
    """NeuralNDCG transposed (allrank/models/losses/neuralNDCG.py:73-136)."""
    a = dict(padded_value_indicator=padded_value_indicator, temperature=temperature, powered_relevancies=powered_relevancies, k=k,
             max_iter=max_iter, tol=tol, **_LOSSES["neuralNDCG_transposed"][1])
    return _neural(y_pred, y_true, a, stochastic, n_samples, beta, log_scores, gumbel)


# ----------------------------------------------------------------------------------------------------------------
# pointwise / pairwise losses
# ----------------------------------------------------------------------------------------------------------------
def rankNet(y_pred, y_true, padded_value_indicator=PADDED_Y_VALUE, weight_by_diff=False, weight_by_diff_powed=False):
    """RankNet (allrank/models/losses/rankNet.py:31-79): BCE-with-logits over the pairs y_i > y_j, mean over all pairs of
    the batch; optional weights |y_i - y_j| or |y_i^2 - y_j^2|."""
    return _call(_RANKNET, y_pred, y_true, dict(padded_value_indicator=padded_value_indicator, weight_by_diff=weight_by_diff,
                                                weight_by_diff_powed=weight_by_diff_powed))


def rankNet_weightByGTDiff(y_pred, y_true, padded_value_indicator=PADDED_Y_VALUE):
    """rankNet.py:8-16"""
    return rankNet(y_pred, y_true, padded_value_indicator, **_LOSSES["rankNet_weightByGTDiff"][1])


def rankNet_weightByGTDiff_pow(y_pred, y_true, padded_value_indicator=PADDED_Y_VALUE):
    """rankNet.py:19-28"""
    return rankNet(y_pred, y_true, padded_value_indicator, **_LOSSES["rankNet_weightByGTDiff_pow"][1])


def bce(y_pred, y_true, padded_value_indicator=PADDED_Y_VALUE):
    """Binary cross-entropy on probabilities (allrank/models/losses/bce.py:8-32): sum over valid items / number of slates
    that contain a valid item."""
    return _call(_BCE, y_pred, y_true, dict(padded_value_indicator=padded_value_indicator, **_LOSSES["bce"][1]))


def with_ordinals(y, n, padded_value_indicator=PADDED_Y_VALUE):
    """ordinal.py:8-22: labels -> [B, L, n] ordinal targets (kept for API parity; the fused loss does not need it)."""
    one_to_n = torch.arange(start=1, end=n + 1, dtype=torch.float, device=y.device)
    unsq = y.unsqueeze(2).repeat(1, 1, n)
    out = (unsq >= one_to_n).type(torch.float)
    out[unsq == padded_value_indicator] = padded_value_indicator
    return out


def ordinal(y_pred, y_true, n, padded_value_indicator=PADDED_Y_VALUE):
    """Ordinal loss (allrank/models/losses/ordinal.py:25-50): y_pred [B, L, n] probabilities, BCE against the ordinal
    targets [y_true >= 1..n], summed / number of valid items."""
    return _call(_BCE, y_pred, y_true, dict(n=int(n), padded_value_indicator=padded_value_indicator), n=int(n))


def pointwise_rmse(y_pred, y_true, no_of_levels, padded_value_indicator=PADDED_Y_VALUE):
    """Pointwise RMSE (allrank/models/losses/pointwise.py:6-32): mean over slates of sqrt(mean (y - levels * p)^2)."""
    return _call(_POINTWISE_RMSE, y_pred, y_true, dict(no_of_levels=no_of_levels, padded_value_indicator=padded_value_indicator))


def binary_listNet(y_pred, y_true, eps=DEFAULT_EPS, padded_value_indicator=PADDED_Y_VALUE):
    """ListNet for binary labels (allrank/models/losses/binary_listNet.py:8-33): target distribution y / sum(y)."""
    return _call(_BINARY_LISTNET, y_pred, y_true, dict(eps=eps, padded_value_indicator=padded_value_indicator))


# ----------------------------------------------------------------------------------------------------------------
# The same launchers for the explicit training step (allrank_amd.engine.FusedTrainer): persistent output / workspace buffers,
# no allocation and no autograd node in run() -> capturable in a hipGraph.
# ----------------------------------------------------------------------------------------------------------------
class FusedLoss(object):
    """``run(scores[B,L], y[B,L], batch_divisor)`` -> (loss[1], dloss/dscores[B,L]) on persistent device buffers.

    ``neuralNDCG`` / ``neuralNDCG_transposed`` with ``stochastic=True`` run here too: ltrx_neuralndcg_prepare on the B slates,
    ltrx_neuralsort_perturb (batch-wide minimum, Gumbel draw, the n_samples * B perturbed pseudo slates with their labels, cut-offs and
    ideal DCGs), ltrx_neuralndcg_fwd_bwd over the pseudo slates, ltrx_neuralsort_fold_grad back onto [B, L].  The noise is a pure
    function of (``set_noise_key``'s seed, its device step word, element index) -- the engine's counter-based generator, not
    torch's -- and the draw of the last ``run`` stays readable in ``self.gumbel`` [n_samples, B, L]."""

    def __init__(self, name, B, SL, device, **args):
        if name not in _LOSSES:
            raise KeyError("no fused launcher for loss %r" % (name,))
        self.name, self.B, self.SL = name, B, SL
        self.fam, fixed = _LOSSES[name]
        # the plugin function's own defaults under the given arguments it knows (others are ignored); KeyError for a missing required one
        params = list(inspect.signature(globals()[name]).parameters.values())[2:]
        a = {p.name: args[p.name] if p.name in args or p.default is p.empty else p.default for p in params}
        self.args = a = dict(a, **fixed)
        if name == "lambdaLoss":
            _check_lambdaloss(a)
        self.stochastic = bool(a.get("stochastic"))
        self.pad, self.eps = float(a["padded_value_indicator"]), float(a.get("eps", DEFAULT_EPS))
        self.bufs = _buffers(self.fam, B, SL, device, a, torch.zeros)
        if self.fam is _LISTMLE:
            self.bufs["perm"] = self.perm = torch.arange(SL, dtype=torch.int64, device=device)
        self.loss, self.ws = self.bufs["loss"], self.bufs["ws"]
        self.grad = torch.zeros((B, SL, int(a["n"])) if a.get("n") else (B, SL), dtype=torch.float32, device=device)
        if self.stochastic:
            self._init_stochastic(device)

    def _init_stochastic(self, device):
        """the persistent buffers of the stochastic form: everything per pseudo slate, the draw, and the S * B-slate workspace"""
        a, B, SL = self.args, self.B, self.SL
        S = self.S = int(a["n_samples"])
        if S < 1:
            raise ValueError("n_samples must be at least 1")

        def new(*shape, dtype=torch.float32):
            return torch.zeros(shape, dtype=dtype, device=device)
        self.s_pert, self.y_ps, self.grad_ps = new(S * B, SL), new(S * B, SL), new(S * B, SL)
        self.k_rows = new(S * B, dtype=torch.int32)
        self.idcg_ps, self.cnt_ps, self.smin = new(S * B), new(1), new(2)
        self.gumbel = new(S, B, SL)
        self._gumbel_given = False
        # the pseudo slates' Sinkhorn call: the transposed form pads under a private sentinel (its gains are the RAW labels)
        self.args_ps = dict(a, padded_value_indicator=-1.0e30) if a["transposed"] else a
        self.ws_ps = torch.empty(max(int(self.fam.ws_bytes(S * B, SL, a)), 64), dtype=torch.uint8, device=device)
        self.ws_stoch = torch.empty(max(int(L.lib().ltrx_neuralsort_stoch_workspace_bytes(B, SL, S)), 64), dtype=torch.uint8, device=device)
        self.set_noise_key(0, torch.zeros(1, dtype=torch.int32, device=device))

    def set_perm(self, perm):
        self.perm.copy_(perm.to(self.perm.device))

    def set_gumbel(self, gumbel):
        """tests: inject the Gumbel draw ([n_samples, B, L] or [n_samples, B, L, 1]) that ``run`` perturbs with instead of drawing;
        None returns to the generator.  (A launch argument: a step captured before the call keeps what it was captured with.)"""
        self._gumbel_given = gumbel is not None
        if gumbel is not None:
            self.gumbel.copy_(gumbel.to(device=self.gumbel.device, dtype=torch.float32).reshape(self.gumbel.shape))

    def set_noise_key(self, seed, step_word):
        """the generator's key: ``seed`` (u32, by value) and ``step_word`` (int32 / u32 [1] on the device, read at every launch -- a
        replayed hipGraph draws fresh noise when the word has moved), folded as the dropout sites fold theirs"""
        self.noise_seed, self.noise_step = int(seed) & 0xFFFFFFFF, step_word

    def _run_stochastic(self, yp, yt):
        a, B, SL, S, lib, P = self.args, self.B, self.SL, self.S, L.lib(), L.ptr
        st = L.stream_of(yp)
        _neural_prepare(yt, a, self.bufs["idcg"], self.bufs["cnt"], self.ws)
        given = self._gumbel_given
        L.check(lib.ltrx_neuralsort_perturb(P(yp), P(yt), P(self.bufs["idcg"]), P(self.bufs["cnt"]), B, SL, S, self.pad, float(a["beta"]),
                                            1 if a["log_scores"] else 0, 1 if a["transposed"] else 0, self.noise_seed,
                                            P(self.noise_step), P(self.gumbel) if given else None, P(self.s_pert), P(self.y_ps),
                                            P(self.k_rows), P(self.idcg_ps), P(self.cnt_ps), P(self.smin),
                                            None if given else P(self.gumbel), P(self.ws_stoch), st), "neuralsort_perturb")
        _launch_neuralndcg(self.s_pert, self.y_ps, self.args_ps, float(S * B), self.loss, self.grad_ps, self.ws_ps, self.idcg_ps,
                           self.cnt_ps, k_rows=None if a["transposed"] else self.k_rows, prepared=True)
        L.check(lib.ltrx_neuralsort_fold_grad(P(self.grad_ps), P(yp), P(self.smin), B, SL, S, 1 if a["log_scores"] else 0, P(self.grad),
                                              P(self.ws_stoch), st), "neuralsort_fold_grad")

    def run(self, yp, yt, batch_divisor=None):
        if self.stochastic:
            self._run_stochastic(yp, yt)
        else:
            self.fam.launch(yp, yt, self.args, float(batch_divisor if batch_divisor is not None else self.B), grad=self.grad, **self.bufs)
        return self.loss, self.grad
