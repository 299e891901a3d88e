"""Ranking on the device: the second entry point of the reference, allrank/rank_and_click.py, on the engine that trained.

The work of that entry point is ``rank_slates`` (allrank/inference/inference_utils.py:14-60): ``model.score`` in eval mode, padded
scores to ``-inf``, a descending sort per slate, a gather of X and y into ranked order.  Here:

  * the scores come from an ``engine.FusedScorer`` -- the forward kernels of the fused step on the VALID rows only, from a padded
    host batch (``run``) or straight from a resident set (``run_resident``);
  * ``ltrx_rank_slates_cu`` (allrank_amd/csrc/ltrx_rank.hip) turns the packed scores into ranked slates padded to L: one workgroup per
    slate sorts in LDS and moves the rows, the tail is 0 / ``PADDED_Y_VALUE``;
  * ``rank_slates(datasets, model, config)`` has the reference's signature and return value, ``{role: (X, y)}`` as CPU tensors;
    ``install(inference=True)`` binds it behind rank_and_click.py:86.

TIES.  The reference sorts with ``torch.sort(descending=True)``, which is not stable: where two items of a slate have exactly the same
score its order is undefined.  This module defines it -- the lower index first, the library's policy (include/ltrx.h) -- on the fused
path and on the module path (``stable=True``) alike.

``last_run`` = {"engine": "fused" | "module", "reason": str}: what the last ``rank_slates`` / ``rank_batches`` call ran, and why the
nn.Module path (``model.score``, ``-inf``, ``torch.sort(stable=True)``, ``gather``) served it where the scorer could not -- a model
the fused engine refuses, ``d_output > 1``, a slate length above LTRX_MAX_METRIC_SLATE_LEN, CPU tensors.  Never an exception.

A model with a positional encoding is scored with ``indices = ones`` for every item (inference_utils.py:47): a quirk of the
reference, reproduced.
"""
import torch

from . import _lib as LB
from .kernels import rank_slates_cu
from .metrics import PADDED_Y_VALUE

__all__ = ["rank_slates", "rank_batches", "rank_slates_cu", "last_run"]

last_run = {"engine": None, "reason": ""}


# ------------------------------------------------------------------------------------------------------------------
# the two engines
# ------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def _module_rank(model, X, y_true):
    """inference_utils.py:44-56 with a stable sort; X [n, L, F], y_true [n, L] on the model's device"""
    mask = y_true == PADDED_Y_VALUE
    scores = model.score(X, mask, torch.ones_like(y_true).type(torch.long))
    scores[mask] = float("-inf")
    _, indices = scores.sort(descending=True, dim=-1, stable=True)
    return torch.gather(X, 1, indices.unsqueeze(-1).expand(-1, -1, X.shape[-1])), torch.gather(y_true, 1, indices)


def padded_batch(slates, ids):
    """the slates ``ids`` of a data.DeviceSlates as a padded batch (xb [n, longest, F], yb [n, longest]) in stored item order --
    features 0 and labels ``PADDED_Y_VALUE`` behind every slate's items, as dataset.py pads; nothing is sampled or permuted"""
    item = slates.item_of[torch.as_tensor(ids, dtype=torch.int64).to(slates.device)]
    rows = item.clamp(min=0)
    xb = torch.where((item >= 0).unsqueeze(-1), slates.x_items[rows], torch.zeros((), device=slates.device))     # (+0.0, never -0.0)
    yb = torch.where(item >= 0, slates.y_items[rows], torch.full((), float(PADDED_Y_VALUE), device=slates.device))
    return xb.contiguous(), yb


class Ranker(object):
    """A model's ranking engine: a FusedScorer per batch shape over the weights of one FusedTrainer -- built from the loaded model at
    the smallest batch, its step never called (the scorer reads the trainer's flat parameters, weight images and transposes) -- plus
    the ranked output buffers.  ``reason`` != "": the fused engine cannot serve this model, every batch takes the module path."""

    def __init__(self, model):
        self.model, self.trainer, self.reason = model, None, ""
        self._scorers, self._out = {}, {}
        try:
            p = next(model.parameters())
        except (StopIteration, AttributeError):
            p = None
        if p is None or not p.is_cuda:
            self.reason = "CPU tensors: the model is not on a GPU"
            return
        if int(getattr(getattr(model, "output_layer", None), "d_output", 1)) > 1:
            self.reason = "d_output > 1: the packed scorer hands out one score per item"
            return
        try:
            from .engine import FusedTrainer
            self.trainer = FusedTrainer(model, "listNet", {}, 1, 8, use_graph=False, fc_step=False)
        except NotImplementedError as e:
            self.reason = "the fused engine refuses the model: %s" % (e,)

    def blocker(self, L):
        """why a batch of slate length ``L`` takes the module path ("" if the scorer serves it)"""
        if self.reason:
            return self.reason
        if L > LB.MAX_METRIC_SLATE_LEN:
            return "a slate length of %d is above LTRX_MAX_METRIC_SLATE_LEN = %d" % (L, LB.MAX_METRIC_SLATE_LEN)
        return ""

    def scorer(self, B, L):
        s = self._scorers.get((B, L))
        if s is None:
            s = self._scorers[(B, L)] = self.trainer.scorer(B, L)
        return s

    def _buffers(self, B, L, F):
        o = self._out.get((B, L, F))
        if o is None:
            dev = self.trainer.dev
            o = self._out[(B, L, F)] = (torch.empty((B, L, F), dtype=torch.float32, device=dev),
                                        torch.empty((B, L), dtype=torch.float32, device=dev))
        return o

    def _rank(self, sc, n, L, F, **source):
        t = self.trainer
        scores, _, cu, order, max_len = sc.packed()
        x_out, y_out = self._buffers(sc.B, L, F)
        # slates 0 .. n-1: the launch order is a STABLE longest-first argsort over the scorer's B slots and the slots past n are empty,
        # so its first n entries are a permutation of the batch's slates
        rank_slates_cu(t.lib, t._st(), scores, cu, order, n, max(max_len, 1), L, x_out, y_out, **source)
        return x_out[:n], y_out[:n]

    def rank_grid(self, B, xb, yb, lengths=None):
        """a padded batch (valid items first in every slate; ``lengths``: host item counts, None = counted on the device)"""
        t = self.trainer
        n, L, F = (int(v) for v in xb.shape)
        sc = self.scorer(max(B, n), L)
        xb = xb.to(t.dev, torch.float32).contiguous()
        yb = yb.to(t.dev, torch.float32).contiguous()
        ones = torch.ones((n, L), dtype=torch.int64, device=t.dev) if t.pos is not None else None
        sc.run(xb, yb, ones, lengths=lengths)
        return self._rank(sc, n, L, F, x=xb, y=yb)

    def rank_resident(self, B, L, slates, ids, lengths):
        """the slates ``ids`` (host int64) of a data.DeviceSlates, padded to ``L``: nothing padded is read"""
        n = int(torch.as_tensor(ids).numel())
        sc = self.scorer(max(B, n), L)
        sc.run_resident(slates, ids, lengths, position=1)
        return self._rank(sc, n, L, slates.n_features, slates=slates, ids=sc.ids)


def _as_ranker(model):
    return model if isinstance(model, Ranker) else Ranker(model)


def _record(engine, reason):
    # (one role on the module path makes the whole call "module": the reason is what a reader needs)
    if last_run["engine"] is None or engine == "module":
        last_run.update(engine=engine, reason=reason)


def _prefix_lengths(yb):
    """host item counts of a padded HOST label batch, or None where padding sits between valid items"""
    valid = yb != PADDED_Y_VALUE
    lens = valid.sum(1, dtype=torch.int32)
    ok = bool((valid == (torch.arange(yb.shape[1])[None, :] < lens[:, None])).all())
    return lens if ok else None


@torch.no_grad()
def _rank_one(rk, batch, B, L):
    if len(batch) == 3:
        slates, ids, lengths = batch
        why = rk.blocker(L)
        if not why:
            _record("fused", "")
            return rk.rank_resident(B, L, slates, ids, lengths)
        dev = next(rk.model.parameters()).device
        xb, yb = (v.to(dev) for v in padded_batch(slates, ids))
    else:
        xb, yb = batch[0], batch[1]
        why = rk.blocker(int(xb.shape[1]))
        lens = None
        if not why and not yb.is_cuda:
            lens = _prefix_lengths(yb)
            why = "" if lens is not None else "padding between the valid items of a slate"
        if not why:
            _record("fused", "")
            return rk.rank_grid(B, xb, yb, lens)
        dev = next(rk.model.parameters()).device
        xb, yb = xb.type(torch.float32).to(dev), yb.to(dev)
    _record("module", why)
    return _module_rank(rk.model, xb, yb)


def rank_batches(model, batches, B, L):
    """Rank ``batches`` with ``model`` (an LTRModel, or a ``Ranker`` kept across calls): yields ``(x_ranked [n, L, F],
    y_ranked [n, L])`` per batch, on the model's device.  A generator: the fused engine's pairs are views of buffers that the NEXT
    batch overwrites.  A batch is ``(xb [n, L, F], yb [n, L])`` -- padded, labels -1 on padding, n <= B, its own L -- or
    ``(slates, ids, lengths)``: slate ids (host int64) of a data.DeviceSlates with their host item counts, every one <= ``L``."""
    rk = _as_ranker(model)
    rk.model.eval()                                           # (and stays in eval mode, as inference_utils.py:40 leaves it)
    for batch in batches:
        yield _rank_one(rk, batch, B, L)


def _resident_set(ds):
    """(DeviceSlates, L) behind a DeviceSlates, a DeviceLibSVMDataset or a packable DeviceLoader; None for anything else"""
    from . import data as ED
    if isinstance(ds, ED.DeviceLoader):
        return (ds.dataset.slates, ds.dataset.longest_query_length) if ds.packable else None
    if isinstance(ds, ED.DeviceLibSVMDataset):
        return ds.slates, ds.longest_query_length
    if isinstance(ds, ED.DeviceSlates):
        return ds, ds.longest_query_length
    return None


def _batches_of(ds, config):
    """(batches for ``rank_batches``, L or None where every batch brings its own) of one role"""
    bs = int(config.data.batch_size)
    res = _resident_set(ds)
    if res is not None:                                       # dataset order, batch_size at a time, padded to the longest slate
        slates, L = res
        ids = torch.arange(slates.n_slates, dtype=torch.int64)
        return ((slates, ids[a:a + bs], slates.lengths_host[a:a + bs]) for a in range(0, slates.n_slates, bs)), L
    from torch.utils.data.dataloader import DataLoader        # the reference's loader settings (inference_utils.py:33-34)
    dl = DataLoader(ds, batch_size=bs, num_workers=config.data.num_workers, shuffle=False)
    return ((xb, yb) for xb, yb, _ in dl), None


def rank_slates(datasets, model, config):
    """Ranks given datasets according to a given model (allrank/inference/inference_utils.py:14-30).

    :param datasets: dictionary of role -> dataset that will be ranked: the reference's LibSVMDataset (iterated with the reference's
        loader settings), or a data.DeviceSlates / DeviceLibSVMDataset / packable DeviceLoader (batched in dataset order,
        ``config.data.batch_size`` slates at a time, padded to the set's longest slate, read straight from HBM)
    :param model: a model to use for scoring documents
    :param config: config for DataLoaders
    :return: dictionary of role -> ranked dataset
        every dataset is a Tuple of torch.Tensor - storing X and y in the descending order of the scores (CPU, float32).
    """
    last_run.update(engine=None, reason="")
    rk = Ranker(model)
    out = {}
    for role, ds in datasets.items():
        batches, L = _batches_of(ds, config)
        xs, ys = [], []
        for xr, yr in rank_batches(rk, batches, int(config.data.batch_size), L):
            xs.append(xr.cpu())
            ys.append(yr.cpu())
        out[role] = (torch.cat(xs), torch.cat(ys))
    if last_run["engine"] is None:
        last_run.update(engine="module" if rk.reason else "fused", reason=rk.reason)
    return out
