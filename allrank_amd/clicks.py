"""Clicks on ranked slates on the device: what allrank/rank_and_click.py does with the slates ``rank_slates`` returned.

  * ``click_on_slates(slates, click_model, include_empty)`` (allrank/click_models/click_utils.py:10-27) -- the reference's signature,
    return value and types; the click model runs in ``ltrx_click_slates_cu`` (allrank_amd/csrc/ltrx_click.hip), one workgroup per slate.
  * ``metrics_on_clicked_slates(clicked_slates)`` (allrank/inference/inference_utils.py:63-82) -- the reference's dicts, computed in
    batches by the ``allrank_amd.metrics`` kernels.
  * ``install(clicks=True)`` binds both behind rank_and_click.py:88 and :95.

CLICK MODELS ON THE DEVICE.  ``plan_of(click_model)`` reads a model into the kernel's arguments.  It takes the specs of this module --
``Cascade``, ``OnlyRelevant``, ``MaxClicks``, ``Diverse`` -- and the reference's objects, recognised by module and class name and read
through their attributes (nothing is imported from the reference):

    [MaxClicksModel(] [DiverseClicksModel(] [MaxClicksModel(] BaseCascadeModel | OnlyRelevantClickModel [)] [)] [)]

Everything else has no plan, and ``plan_of`` says why: Random / Fixed / Multiple / Conditioned click models,
EverythingButDuplicatesClickModel on its own, a Diverse inside a Diverse, an unknown class.

GENERATOR.  Host draws come from the GLOBAL numpy generator exactly as the reference consumes it: a cascade draws
``np.random.rand(n)`` per slate, in slate order, which is ONE ``np.random.rand(total valid items)`` per call; OnlyRelevant draws nothing.
After the call ``np.random.get_state()`` equals the reference's.  The position table ``1 / np.arange(1, L + 1) ** eta`` is numpy's, on
the host (cascade_models.py:31), uploaded as fp64; the compare ``table >= u`` is the kernel's, in fp64.

TIES AND ARITHMETIC.  include/ltrx.h states the distance (sequential fp64, no FMA, one stored value for the quantile and the
comparisons).  On data without exact ties at the margin the clicks equal the reference's (scipy's cdist, np.quantile).

CHUNKS.  Slates go to the device ``CHUNK_BYTES`` (256 MiB) of padded features at a time, at least one slate; the result does not depend
on the chunking.

HOST PATH.  A model without a plan, a slate with padding between valid items, a slate length above the kernel's limits
(LTRX_MAX_SLATE_LEN for a diverse model, LTRX_MAX_METRIC_SLATE_LEN otherwise) or no GPU: the call runs on the host with the reference's
semantics -- the original ``click_on_slates`` that install() kept, else a per-slate loop over ``click_model.click`` with
MaskedRemainMasked's masking.  ``last_run`` = {"engine": "device" | "host", "reason": str}.  Never an exception for that reason.
"""
import numpy as np
import torch

from . import _lib as LB
from .kernels import click_slates_cu
from .metrics import PADDED_Y_VALUE

__all__ = ["Cascade", "OnlyRelevant", "MaxClicks", "Diverse", "plan_of", "click_on_slates", "metrics_on_clicked_slates",
           "click_slates_cu", "last_run"]

last_run = {"engine": None, "reason": ""}
CHUNK_BYTES = 256 << 20          # padded feature bytes of one upload
METRIC_BATCH = 4096              # slates of one metric launch
_reference = {}                  # the reference's own functions, kept by install(clicks=True): name -> function


# ------------------------------------------------------------------------------------------------------------------
# the specs: small click models of our own, with the reference's host semantics in numpy (``click``) so that the host path serves them
# ------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def pairwise_distances(X):
    """[n, n] Euclidean distances of the rows of X in the arithmetic of the kernel: fp64, squares added over k ascending"""
    X = _np(X).astype(np.float64)
    s = np.zeros((X.shape[0], X.shape[0]), dtype=np.float64)
    for k in range(X.shape[1]):
        d = X[:, None, k] - X[None, :, k]
        s += d * d
    return np.sqrt(s)


def duplicate_margin(dist, q):
    """np.quantile of the pairs i < j of a distance matrix (cascade_models.py:57-60, :70-73); 0 without a pair"""
    n = dist.shape[0]
    if n < 2:
        return 0.0
    return np.quantile(dist[np.triu_indices(n, 1)], q=q)


class Cascade(object):
    """BaseCascadeModel: position i is observed iff 1 / (i + 1) ** eta >= a uniform draw; clicked iff y * observed >= threshold"""

    def __init__(self, eta, threshold):
        self.eta, self.threshold = eta, threshold

    def click(self, documents):
        _, y = documents
        y = _np(y)
        observed = (1 / np.arange(1, len(y) + 1) ** self.eta) >= np.random.rand(len(y))
        return np.where(observed, y, y.dtype.type(0)) >= self.threshold


class OnlyRelevant(object):
    """OnlyRelevantClickModel: clicked iff y >= threshold"""

    def __init__(self, threshold):
        self.threshold = threshold

    def click(self, documents):
        return _np(documents[1]) >= self.threshold


class MaxClicks(object):
    """MaxClicksModel: the first ``max_clicks`` clicks of ``inner`` (None: all of them)"""

    def __init__(self, inner, max_clicks):
        self.inner, self.max_clicks = inner, max_clicks

    def click(self, documents):
        c = self.inner.click(documents)
        return c if self.max_clicks is None else c * (c.cumsum() <= self.max_clicks)


class Diverse(object):
    """DiverseClicksModel: the clicks of ``inner`` in rank order, each kept iff farther than the ``q_percentile`` quantile of all
    pairwise distances from every click kept so far"""

    def __init__(self, inner, q_percentile=0.5):
        self.inner, self.q_percentile = inner, q_percentile

    def click(self, documents):
        X, _ = documents
        dist = pairwise_distances(X)
        margin = duplicate_margin(dist, self.q_percentile)
        c = np.array(self.inner.click(documents), dtype=bool)
        kept = []
        for i in np.flatnonzero(c):
            if all(dist[j, i] > margin for j in kept):
                kept.append(i)
            else:
                c[i] = False
        return c


_REF = "allrank.click_models."
_KINDS = {Cascade: "cascade", OnlyRelevant: "relevant", MaxClicks: "max", Diverse: "diverse"}
_REF_KINDS = {_REF + "cascade_models.BaseCascadeModel": "cascade", _REF + "base.OnlyRelevantClickModel": "relevant",
              _REF + "base.MaxClicksModel": "max", _REF + "cascade_models.DiverseClicksModel": "diverse"}


def _read(m):
    """(kind, fields) of one layer of a click model, or (None, reason)"""
    name = type(m).__module__ + "." + type(m).__name__
    kind = _KINDS.get(type(m)) or _REF_KINDS.get(name)
    ours = type(m) in _KINDS
    if kind == "cascade":
        return kind, (m.eta, m.threshold)
    if kind == "relevant":
        return kind, (m.threshold if ours else m.relevancy_threshold,)
    if kind == "max":
        return kind, (m.inner if ours else m.inner_click_model, m.max_clicks)
    if kind == "diverse":
        return kind, (m.inner if ours else m.inner_click_model, m.q_percentile)
    return None, "%s has no device form" % name


def plan_of(click_model):
    """(plan, "") -- the kernel arguments of a click model, a dict with ``kind`` ("cascade" | "relevant"), ``eta``, ``threshold``,
    ``max_candidates``, ``diverse``, ``q``, ``max_clicks`` (-1: no limit) -- or (None, reason)"""
    plan = dict(kind=None, eta=None, threshold=None, max_candidates=-1, diverse=0, q=0.0, max_clicks=-1)
    m = click_model
    while True:
        kind, f = _read(m)
        if kind is None:
            return None, f
        if kind == "max":
            if f[1] is not None:
                if int(f[1]) != f[1] or f[1] < 0:
                    return None, "max_clicks = %r is no count" % (f[1],)
                key = "max_candidates" if plan["diverse"] else "max_clicks"
                plan[key] = int(f[1]) if plan[key] < 0 else min(plan[key], int(f[1]))
            m = f[0]
        elif kind == "diverse":
            if plan["diverse"]:
                return None, "a diverse model inside a diverse model has no device form"
            q = float(f[1])
            if not 0.0 <= q <= 1.0:
                return None, "q_percentile = %r is outside [0, 1]" % (f[1],)
            plan.update(diverse=1, q=q)
            m = f[0]
        else:
            thr = float(f[-1])
            if float(np.float32(thr)) != thr:
                return None, "a threshold of %r is no float32 value" % (f[-1],)
            plan.update(kind=kind, threshold=thr, eta=f[0] if kind == "cascade" else None)
            return plan, ""


# ------------------------------------------------------------------------------------------------------------------
# click_on_slates
# ------------------------------------------------------------------------------------------------------------------
def _host_clicks(X, y, click_model):
    """click_utils.py:21 on the host: MaskedRemainMasked(click_model).click per slate"""
    X, y = (v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v)) for v in (X, y))
    out = []
    for Xs, ys in zip(X, y):
        mask = ys == PADDED_Y_VALUE
        c = click_model.click((Xs[~mask], ys[~mask]))
        final = np.zeros_like(ys.numpy())
        final[mask.numpy()] = PADDED_Y_VALUE
        final[~mask.numpy()] = c
        out.append(final)
    return out


def _filtered(X, clicks, include_empty):
    kept = [(X[s], c) for s, c in enumerate(clicks) if (np.sum(c > 0) > 0 or include_empty)]
    return_X, kept_clicks = map(list, zip(*kept))             # nothing kept: the reference's ValueError
    return return_X, kept_clicks


def _blocker(plan, y):
    """(reason a call with a plan takes the host path or "", host item counts)"""
    if not torch.cuda.is_available():
        return "no GPU", None
    valid = y != PADDED_Y_VALUE
    lens = valid.sum(1)
    if not bool((valid == (torch.arange(y.shape[1], device=y.device)[None, :] < lens[:, None])).all()):
        return "padding between the valid items of a slate", None
    lens = lens.cpu().numpy().astype(np.int64)
    longest = int(lens.max()) if lens.size else 0
    limit, name = (LB.MAX_SLATE_LEN, "LTRX_MAX_SLATE_LEN") if plan["diverse"] else (LB.MAX_METRIC_SLATE_LEN, "LTRX_MAX_METRIC_SLATE_LEN")
    if longest > limit:
        return "a slate of %d items is above %s = %d" % (longest, name, limit), None
    return "", lens


def _device_clicks(X, y, plan, lens, margins=None):
    """the clicks [N, L] (float32 numpy) of ``plan``; ``margins``: an fp64 numpy array [N] to fill (the kernel then computes every
    slate's margin), None in the product path"""
    N, L, F = (int(v) for v in X.shape)
    dev = X.device if X.is_cuda else torch.device("cuda", torch.cuda.current_device())
    lib, st = LB.lib(), LB.launch_stream(dev)
    u_all = table = None
    if plan["kind"] == "cascade":
        u_all = np.random.rand(int(lens.sum()))               # the reference's per-slate rand(n) draws, concatenated
        table = torch.from_numpy(np.asarray(1 / np.arange(1, L + 1) ** plan["eta"], dtype=np.float64)).to(dev)
    starts = np.concatenate([[0], np.cumsum(lens)])
    per = max(1, int(CHUNK_BYTES // max(1, L * F * 4)))
    clicks = np.empty((N, L), dtype=np.float32)
    for a in range(0, N, per):
        b = min(a + per, N)
        n = b - a
        xb = X[a:b].to(dev, torch.float32).contiguous()
        yb = y[a:b].to(dev, torch.float32).contiguous()
        ln = lens[a:b]
        cu = torch.from_numpy(np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)).to(dev)
        order = torch.from_numpy(np.argsort(-ln, kind="stable").astype(np.int32)).to(dev)
        max_len = max(int(ln.max()), 1)
        u = None
        if u_all is not None:                                 # (a chunk without a valid item still hands the kernel a non-NULL u)
            seg = u_all[starts[a]:starts[b]]
            u = torch.from_numpy(seg if seg.size else np.zeros(1)).to(dev)
        out = torch.empty((n, L), dtype=torch.float32, device=dev)
        mg = torch.empty((n,), dtype=torch.float64, device=dev) if margins is not None else None
        nbytes = lib.ltrx_click_workspace_bytes(n, max_len, plan["diverse"])
        ws = LB.workspace(nbytes, xb) if nbytes else None
        click_slates_cu(lib, st, xb, yb, cu, order, n, max_len, out, plan, u, table, mg, ws)
        clicks[a:b] = out.cpu().numpy()
        if margins is not None:
            margins[a:b] = mg.cpu().numpy()
    return clicks


def click_on_slates(slates, click_model, include_empty):
    """
    This metod runs a click model on a list of slates and returns new slates with `y` taken from clicks
    (allrank/click_models/click_utils.py:10-27)

    :param slates: a Tuple of X, y (CPU or device tensors, or arrays):
        X being a list of slates represented by document vectors [N, L, F]
        y being a list of slates represented by document relevancies [N, L], -1 on padding
    :param click_model: a click model to be applied to every slate
    :param include_empty: if True - will return even slates that didn't get any click
    :return: Tuple of X, clicks, X representing the same document vectors as input 'X', clicks representing click mask for every slate
        (float32 numpy vectors of length L: 1 clicked, 0 not clicked, -1 padding)
    """
    X, y = slates
    plan, why = plan_of(click_model)
    lens = None
    if plan is not None:
        Xt, yt = (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v)) for v in (X, y))
        if Xt.dim() != 3 or yt.dim() != 2 or Xt.shape[:2] != yt.shape or 0 in Xt.shape:
            why = "slates that are no [N, L, F] / [N, L] pair"
        else:
            why, lens = _blocker(plan, yt)
    if why:
        last_run.update(engine="host", reason=why)
        ref = _reference.get("click_on_slates")
        if ref is not None and not (torch.is_tensor(X) and X.is_cuda):    # (the reference's numpy calls take host tensors)
            return ref(slates, click_model, include_empty)
        return _filtered(X, _host_clicks(X, y, click_model), include_empty)
    last_run.update(engine="device", reason="")
    clicks = _device_clicks(Xt, yt, plan, lens)
    return _filtered(X, list(clicks), include_empty)


# ------------------------------------------------------------------------------------------------------------------
# metrics_on_clicked_slates
# ------------------------------------------------------------------------------------------------------------------
def _host_dcg_ndcg(c):
    """dcg and ndcg (ats=None, gain 2^y - 1, filler 1.0) of click vectors c [n, L] already in ranked order, padding last: metrics.py's
    float32 torch operations on the host (padded labels count as 0, a running sum over the positions)"""
    y = torch.from_numpy(c).clamp(min=0)
    disc = torch.tensor(1.0) / torch.log2(torch.arange(c.shape[1], dtype=torch.float) + 2.0)
    dcg = torch.cumsum((torch.pow(2, y) - 1) * disc, dim=1)[:, -1]
    ideal = torch.cumsum((torch.pow(2, y.sort(descending=True, dim=1)[0]) - 1) * disc, dim=1)[:, -1]
    ndcg = torch.where(ideal == 0, torch.ones_like(dcg), dcg / torch.where(ideal == 0, torch.ones_like(ideal), ideal))
    return dcg.numpy(), ndcg.numpy()


def metrics_on_clicked_slates(clicked_slates):
    """inference_utils.py:73-82: per clicked slate {"slate_length", "no_of_clicks", "dcg", "ndcg"}, y_pred the descending ramp L .. 1,
    y_true the clicks, ats=None.  Slates are grouped by length and go through ``allrank_amd.metrics`` METRIC_BATCH at a time (float32
    results, within the metric contract of 1e-5 of the reference's).  Without a GPU, or above LTRX_MAX_METRIC_SLATE_LEN, the call runs
    on the host: the reference's own generator where install() kept it, else metrics.py's operations restated in torch."""
    from . import metrics as EM
    _, ys = clicked_slates
    ys = [_np(v) for v in ys]
    gpu = torch.cuda.is_available()
    ref = _reference.get("metrics_on_clicked_slates")
    if ref is not None and (not gpu or any(len(v) > LB.MAX_METRIC_SLATE_LEN for v in ys)):
        yield from ref(clicked_slates)
        return
    dcgs, ndcgs = np.empty(len(ys)), np.empty(len(ys))
    groups = {}
    for s, v in enumerate(ys):
        groups.setdefault(len(v), []).append(s)
    for L, ids in groups.items():
        if L == 0:
            dcgs[ids], ndcgs[ids] = 0.0, 1.0
            continue
        for a in range(0, len(ids), METRIC_BATCH):
            part = ids[a:a + METRIC_BATCH]
            c = np.stack([ys[s] for s in part]).astype(np.float32)
            if gpu and L <= LB.MAX_METRIC_SLATE_LEN:
                yt = torch.from_numpy(c).cuda()
                yp = torch.arange(L, 0, -1, dtype=torch.float32, device=yt.device)[None, :].expand(len(part), L)
                nd, dc, _ = EM._run(yp, yt, None, PADDED_Y_VALUE, 1.0, False)
                dcgs[part], ndcgs[part] = dc[:, 0].cpu().numpy(), nd[:, 0].cpu().numpy()
            else:
                dcgs[part], ndcgs[part] = _host_dcg_ndcg(c)
    for s, v in enumerate(ys):
        yield {"slate_length": len(v), "no_of_clicks": np.int64((v > 0).sum()), "dcg": float(dcgs[s]), "ndcg": float(ndcgs[s])}
