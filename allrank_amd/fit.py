"""The epoch loop of allRank with the reference's own signature -- ``fit`` of allrank/training/train_utils.py:78-147 -- so that
``allrank_amd.install(fit=True)`` puts the explicit MI355X training step (engine.FusedTrainer) behind an UNMODIFIED
``allrank/main.py`` (main.py:90 calls ``fit(model=..., loss_func=..., optimizer=..., scheduler=..., train_dl=..., valid_dl=...,
config=..., device=..., output_dir=..., tensorboard_output_path=..., **asdict(config.training))``).

What is kept from the reference loop: the arguments and their meaning, per-epoch order (train pass, validation pass, scheduler
step incl. ReduceLROnPlateau on ``config.val_metric``, early stopping with EarlyStop's rule, early_stop.py:7-19), gradient clipping,
the ``model.pkl`` state_dict written to ``output_dir`` (loadable by the reference: same keys and shapes), tensorboard scalars when the
reference's writer is importable, and the returned dict {"epochs", "train_metrics", "val_metrics", "num_params"}.

What changes (all outside the arithmetic of a step):
  * a training step is ``FusedTrainer.step`` (hand-written HIP forward/backward/Adam, hipGraph replay) when the model family, the
    loss and the optimizer allow it (``_fused_spec``) and the autograd ``Trainer`` (same kernels for attention / LayerNorm / loss,
    torch autograd + the given optimizer) otherwise.  The two engines offer the loop the same members (engine.Trainer's docstring);
    after the construction block ``fit()`` talks to "the trainer" and does not ask which one it is;
  * host batches are copied on a separate stream one batch ahead (``_Prefetcher``) instead of ``.to(device)`` per step (:95);
  * no ``loss.item()`` per step: the running loss is accumulated on the device, one host sync per epoch (train_utils.py:29);
  * a validation batch is scored by one of four sources (``_score_batch``): the forward half of the explicit step where the batch
    has the training shape, else the nn.Module forward; with ``val_scorer="packed"`` / ``"ragged"`` the packed, captured
    forward-only scorer (engine.FusedScorer), fed from the resident set or from the padded batch (fit()'s docstring);
  * train metrics come from the scores of the training forward itself instead of a second full pass over ``train_dl`` in train()
    mode (train_utils.py:99; same mode, same data).  ``train_metrics="reference"`` (or the environment variable
    ALLRANK_AMD_TRAIN_METRICS=reference) runs the reference's second pass instead: one pass over ``train_dl`` per metric name with
    the END-of-epoch weights (dropout is off in that pass; the reference leaves it on, so its numbers carry that noise);
  * the loaders' draws from torch's global generator stay in step with the reference's loop, which iterates ``train_dl`` and
    ``valid_dl`` 1 + (number of metric names) times per epoch (train_utils.py:95-107, :36-43): the passes skipped here are replaced by
    ``_burn``, so under main.py:36-38's seeds epoch e trains on the reference's batches in the reference's order;
  * batches that are already on the device pass straight through (``allrank_amd.data.DeviceLoader``, bound behind main.py:57-68 by
    install()); under a process group such a loader yields only this rank's block of each global batch (``ShardBatch``);
  * ``config.detect_anomaly`` (main.py:89; the explicit step has no autograd graph for torch's anomaly mode to watch) or
    LTRX_CHECK_FINITE=1: ``_assert_finite`` after every step (one host sync) names the first offending parameter tensor;
  * the last, short batch of an epoch (DataLoader drop_last=False) trains as it is delivered (``step_block``: the fused engine tops
    it up with fully padded slates for its static shape); its loss is normalised by the real slate count;
  * under an initialised ``torch.distributed`` group every rank takes its contiguous block of each global batch, training AND
    validation (the reference wraps the model in nn.DataParallel instead, main.py:76-78; such a wrapper passed in is unwrapped);
  * ``checkpoint_every`` / ``resume``: the whole state of the run can be written to ``output_dir/checkpoint.pt`` at epoch boundaries
    and a stopped job continued as the same job, bit for bit (fit()'s docstring, allrank_amd.checkpoint).  Off by default.
"""
import collections
import contextlib
import functools
import logging
import os
import time

import numpy as np
import torch

from . import checkpoint as CK
from . import losses as E
from . import metrics as EM
from . import ragged as RG
from .data import ShardBatch
from .engine import FusedTrainer, Trainer, PADDED_Y_VALUE, pad_batch as _pad_batch
from .parallel import shard_slates

log = logging.getLogger("allrank_amd.fit")

NORMALIZATION_FILE = "feature_normalization.npz"      # beside model.pkl when the training data set carries a FeatureNormalizer

last_run = {}          # what the most recent fit() used: {"engine": "fused" | "autograd", "compact": bool, "reason": str,
#                        "sampling": the training DeviceLoader's mode ("device" | "reference"; None for any other loader),
#                        "compact_graph": what the captured variable-length step did (None: off), "compact_graph_reason": str, ...;
#                        "normalize": {"roles", "log", "no_log_negative"} only when the training data set carries a normaliser}


class _EarlyStop(object):
    """allrank/training/early_stop.py:7-19"""

    def __init__(self, patience):
        self.patience, self.best_value, self.best_epoch = patience, 0.0, 0

    def step(self, current_value, current_epoch):
        if current_value > self.best_value:
            self.best_value, self.best_epoch = current_value, current_epoch

    def stop_training(self, current_epoch):
        return current_epoch - self.best_epoch > self.patience


def _tensorboard(path):
    try:
        from allrank.utils.tensorboard_utils import TensorboardSummaryWriter
        return TensorboardSummaryWriter(path)
    except Exception:
        return None


def _fused_spec(model, loss_func, optimizer):
    """(loss_name, loss_args, lr, optimizer kwargs of FusedTrainer) if the explicit step can run this job, else (None, reason)"""
    from .model import LTRModel
    if not isinstance(model, LTRModel):
        return None, "model is not an allrank_amd LTRModel"
    if not isinstance(loss_func, functools.partial) or getattr(E, getattr(loss_func.func, "__name__", ""), None) is not loss_func.func:
        return None, "loss is not a functools.partial of an allrank_amd loss"
    if loss_func.args:
        return None, "positional loss arguments"
    if len(optimizer.param_groups) != 1:
        return None, "optimizer has several parameter groups"
    g = optimizer.param_groups[0]
    if g.get("maximize", False) or g.get("amsgrad", False):
        return None, "maximize / amsgrad"
    if type(optimizer) in (torch.optim.Adam, torch.optim.AdamW):
        opt = dict(optimizer=type(optimizer).__name__, betas=tuple(g["betas"]), eps=float(g["eps"]), weight_decay=float(g["weight_decay"]))
    elif type(optimizer) is torch.optim.SGD:
        if g.get("dampening", 0) != 0:
            return None, "SGD with dampening"
        opt = dict(optimizer="SGD", momentum=float(g["momentum"]), nesterov=bool(g["nesterov"]), weight_decay=float(g["weight_decay"]))
    else:
        return None, "optimizer %s is not one of the fused Adam / AdamW / SGD" % type(optimizer).__name__
    return (loss_func.func.__name__, dict(loss_func.keywords or {}), float(g["lr"]), opt), ""


class _Prefetcher(object):
    """Host batches -> device batches with one batch of look-ahead.  The reference copies every batch on the compute stream in
    front of the step (``xb.to(device)``, train_utils.py:95).  Here batch t+1 is copied on a SEPARATE stream into one of two
    persistent device sets while the GPU runs step t (as soon as the step that last read that set has finished), and the compute
    stream waits for the copy's event before step t+1.  Measured at config 3 (tools/fit_h2d_timing.py, 34 MB per batch): batch
    resident in HBM 9.9 ms per step, ``.to(device)`` per step 10.8 ms, this class 10.65-10.7 ms -- the host-to-device copy executes as
    a blit kernel that shares the CUs with the step, so most of its 0.8 ms stays; an extra hop through pinned staging buffers
    costs 5+ ms of host time per batch on this platform (15-17 ms per step) and is not used.  Keeping the training set in HBM
    (allrank_amd.data.DeviceSlates) is what removes the copy.  Batches that are already on the device pass through."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.stage = [None, None]          # per set: (device tensors, event "copy done")
        self.free = [None, None]           # per set: event on the compute stream "the step that read this device set has finished"
        self.turn = 0

    def _send(self, batch):
        if all((not torch.is_tensor(t)) or t.is_cuda for t in batch):
            return batch, None, None
        k = self.turn & 1
        self.turn += 1
        slot = self.stage[k]
        if slot is None or any(d.shape[1:] != t.shape[1:] or d.shape[0] < t.shape[0] or d.dtype != t.dtype for d, t in zip(slot[0], batch)):
            torch.cuda.current_stream(self.device).synchronize()      # (re)allocation: nothing of the old set may still be in use
            slot = self.stage[k] = ([torch.empty(t.shape, dtype=t.dtype, device=self.device) for t in batch], torch.cuda.Event())
            self.free[k] = None
        dev, ev = slot
        n = batch[0].shape[0]
        if self.free[k] is not None:
            self.stream.wait_event(self.free[k])
        with torch.cuda.stream(self.stream):
            for t, d in zip(batch, dev):
                d[:n].copy_(t, non_blocking=True)
            ev.record(self.stream)
        return [d[:n] for d in dev], ev, k

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._send(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur, ev, k = nxt
            if ev is not None:
                torch.cuda.current_stream(self.device).wait_event(ev)
            yield cur
            if k is not None:                             # the consumer has enqueued its work on the compute stream
                e = torch.cuda.Event()
                e.record(torch.cuda.current_stream(self.device))
                self.free[k] = e
            try:
                nxt = self._send(next(it))
            except StopIteration:
                nxt = None


def make_result(epoch, train_metrics, val_metrics, num_params):
    """the dict main.py:90 receives, with the VALUE TYPES the reference's fit returns: main.py:104 hands it to
    dump_experiment_result (utils/experiments.py:20-24), which calls ``.item()`` on every metric and on num_params -- numpy scalars in
    the reference (np.mean in train_utils.py:38-43, np.sum in model_utils.py:21-28), so numpy scalars here"""
    return {"epochs": epoch,
            "train_metrics": {k: np.float64(v) for k, v in train_metrics.items()},
            "val_metrics": {k: np.float64(v) for k, v in val_metrics.items()},
            "num_params": np.int64(num_params)}


def _batch_shape(dl):
    """(slates per batch, slate length) of a loader without consuming a batch: DataLoader.batch_size and the shape of one dataset
    item ([L, F] features, dataset_loading.py:19-29); loaders that do not expose them are asked for their first batch instead.
    Also returns the fraction of valid (non-padded) slots over a sample of the set (the auto choice of variable-length execution)."""
    if hasattr(dl, "batch_shape"):                  # allrank_amd.data.DeviceLoader knows all three without touching a batch
        return dl.batch_shape()
    try:
        bsz, ds = int(dl.batch_size), dl.dataset
        # The probe indexes dataset items; the reference's FixLength transform draws from the GLOBAL numpy generator when it
        # subsamples a long slate (dataset_loading.py:70), so the generator state is saved and restored around it -- a seeded run draws
        # the same subsamples with and without the probe.
        st = np.random.get_state()
        try:
            items = [ds[i] for i in range(0, len(ds), max(1, len(ds) // 32))][:32]
        finally:
            np.random.set_state(st)
        ys = torch.stack([torch.as_tensor(it[1]).float() for it in items])
        return bsz, int(items[0][0].shape[0]), float((ys != PADDED_Y_VALUE).float().mean())
    except (AttributeError, TypeError, IndexError, KeyError):          # loaders without batch_size / an indexable dataset
        first = next(iter(dl))
        return int(first[0].shape[0]), int(first[0].shape[1]), float((first[1] != PADDED_Y_VALUE).float().mean())


def _check_same_batch(xb, yb, world, batch=None):
    """sharded runs: every rank must see the SAME global batch for shard_slates to partition it (the reference's DataLoader
    shuffles per process; give the ranks one sampler seed) -- checked on the first batch with an all-gathered checksum.  A
    ``ShardBatch`` that is already this rank's block carries the checksum of the global batch's slate ids instead."""
    import torch.distributed as dist
    if batch is not None:
        chk = torch.tensor([float(batch.order_tag & 0xFFFFFF), float(batch.order_tag >> 24), float(batch.global_slates)], device=xb.device,
                           dtype=torch.float64)
    else:
        chk = torch.stack([xb.double().sum(), yb.double().sum(), torch.tensor(float(xb.shape[0]), device=xb.device, dtype=torch.float64)])
    allc = [torch.empty_like(chk) for _ in range(world)]
    dist.all_gather(allc, chk)
    if any(not torch.equal(c, allc[0]) for c in allc):
        raise RuntimeError("allrank_amd.fit: the ranks received different first batches -- under torch.distributed every rank must "
                           "iterate the same global batches (same DataLoader sampler seed / shuffle order); rank r trains on its "
                           "contiguous block of each of them")


def _my_block(batch, loader, rank, world):
    """(xb, yb, idx, slates in the global batch, the ShardBatch if the loader has already cut this rank's block) of one loader item"""
    xb, yb, idx = batch
    pre = isinstance(batch, ShardBatch) and world > 1 and getattr(loader, "world", 1) == world
    n_glob = batch.global_slates if isinstance(batch, ShardBatch) else int(xb.shape[0])
    if world > 1 and not pre:
        a, b = shard_slates(n_glob, rank, world)
        xb, yb, idx = xb[a:b], yb[a:b], idx[a:b]
    return xb, yb, idx, n_glob, (batch if pre else None)


def _host_lengths(batch, real, pre, world):
    """valid items per slate of this rank's block as HOST integers -- what variable-length execution needs to size its launches
    without a device round trip (allrank_amd/rows.py).  A DeviceLoader knows them (the slate lengths of the resident set), and they
    are usable where they are those of this rank's ``real`` slates; any other loader: None (counted on the device, one host sync)."""
    lens = getattr(batch, "lengths", None)
    return lens if lens is not None and (pre is not None or world == 1) and int(lens.numel()) == real else None


def _compact_mode(compact):
    """fit()'s ``compact`` argument resolved: None (choose by the share of valid slots), False, True, or "graph" -- the captured
    variable-length step, which an unmodified main.py asks for with ALLRANK_AMD_COMPACT=graph (the only value the variable takes;
    it is read when the argument is None)"""
    if compact is None:
        env = os.environ.get("ALLRANK_AMD_COMPACT")
        if not env:
            return None
        if env.lower() != "graph":
            raise ValueError("ALLRANK_AMD_COMPACT must be 'graph' (or unset), got %r" % (env,))
        return "graph"
    if isinstance(compact, str):
        if compact.lower() != "graph":
            raise ValueError("compact must be None, False, True or 'graph', got %r" % (compact,))
        return "graph"
    return bool(compact)


def _compact_graph_stats(trainer):
    """last_run["compact_graph"]: what the captured variable-length step did so far (None: the mode is not active)"""
    if not getattr(trainer, "compact_graph", False):              # (tools hand it objects that are no trainer)
        return None
    c = trainer.mode_counts
    return {"buckets": dict(sorted(trainer.bucket_counts.items())), "captures": c["capture"], "replays": c["replay"],
            "eager_steps": c["eager"], "evictions": trainer._step_graphs.evictions}


def _burn(dl, times=1):
    """Consume what ``times`` iterations over ``dl`` draw from torch's global generator without loading a batch: the worker base
    seed every ``iter(DataLoader)`` draws and the seed a RandomSampler draws at its first index (torch/utils/data/dataloader.py,
    sampler.py) -- the passes of the reference's epoch loop that this loop does not make (module docstring)."""
    from torch.utils.data import DataLoader
    for _ in range(times):
        if hasattr(dl, "burn"):
            dl.burn()
        elif isinstance(dl, DataLoader) and dl.batch_sampler is not None:
            iter(DataLoader(dl.dataset, batch_sampler=dl.batch_sampler, num_workers=0, generator=dl.generator))   # the base seed (no
            #                                                                                   worker is started, no item is loaded)
            next(iter(dl.sampler), None)                                                     # the sampler's seed / permutation draw
        else:
            return False
    return True


def _packed_blocker(loss_func, fused, reason):
    """why the packed validation scorer cannot serve this job ("" if it can)"""
    name = getattr(getattr(loss_func, "func", None), "__name__", "")
    if name in ("neuralNDCG", "neuralNDCG_transposed") and (getattr(loss_func, "keywords", None) or {}).get("stochastic"):
        # loss_utils.py:102 takes the batch-wide minimum over the PADDED scores too (and draws noise at validation): the value depends
        # on what sits in the padded slots, which the packed scorer sets to 0 and the nn.Module forward does not
        return "stochastic NeuralNDCG reads padded scores (batch-wide min, loss_utils.py:102)"
    if not fused:
        return "no FusedTrainer (%s)" % (reason or "autograd step")
    return ""


def _val_scorer(scorers, trainer, n, L):
    """the FusedScorer for validation batches of up to n slates of L items (one per slate length, grown if a batch is larger)"""
    s = scorers.get(L)
    if s is None or s.B < n:
        s = scorers[L] = trainer.scorer(max(n, 1), L)
    return s


def _ragged_plan(loss_func, trainer, metrics):
    """what fit(val_scorer="ragged") evaluates on the packed rows: {"loss": the ragged form of ``loss_func`` or None, "metrics": the
    metric names with a ragged form}.  A model with d_output > 1 (ordinal) keeps everything on the padded grid: its loss reads
    [B, L, d_output] scores."""
    if getattr(trainer, "n_out", 1) != 1:
        return {"loss": None, "metrics": ()}
    return {"loss": RG.form_of(loss_func) if loss_func is not None else None,
            "metrics": tuple(name for name in metrics if RG.form_of(getattr(EM, name, None)) is not None)}


class _EpochStats(object):
    """What an epoch's pass adds up on this rank -- its detached fp32 share of each global batch's loss x that batch's slates, its own
    slates, per-metric sums over slates -- and the ONE ``cat`` / ``all_reduce`` / host copy that ends the pass."""

    def __init__(self, metrics, device):
        self.metrics, self.device = metrics, device
        self.tot, self.num, self.sums = torch.zeros((), device=device), 0, {name: None for name in metrics}

    def add(self, share, n_glob, n):
        self.tot += share.reshape(()) * n_glob
        self.num += n

    def add_metric(self, name, v):
        self.sums[name] = v if self.sums[name] is None else self.sums[name] + v

    def finish(self, world, zero_fill):
        """(loss sum, slate count, {"name_at": sum}) over all ranks, as the fp32 numpy scalars of the host copy.  A metric never added
        is left out (training under train_metrics="reference") or, ``zero_fill``, counts as zeros (validation: every rank one layout)."""
        names = [name for name in self.metrics if zero_fill or self.sums[name] is not None]
        sums = [self.sums[name].float() if self.sums[name] is not None else torch.zeros(len(self.metrics[name]), device=self.device)
                for name in names]
        stats = torch.cat([self.tot.reshape(1), torch.tensor([float(self.num)], device=self.device)] + sums)
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(stats)
        stats = stats.cpu().numpy()
        return stats[0], stats[1], dict(zip(["%s_%d" % (name, at) for name in names for at in self.metrics[name]], stats[2:]))


# one validation batch as its score source left it: ``scores`` [n, L] and ``y`` (first n rows) for the padded metrics, ``out`` and
# ``labels`` (max(n, 1) slates) for the padded loss, ``n`` of ``n_glob`` slates, ``packed``: the scorer that ran (ragged plan) or None
_ValBatch = collections.namedtuple("_ValBatch", "scores y out labels n n_glob packed")


def _score_batch(batch, loader, resident, model, trainer, scorers, ragged, world, rank):
    """Score one validation batch through the one source that serves it: a FusedScorer fed from the resident set (``resident``) or
    from the padded batch (``scorers``; slates above LTRX_MAX_METRIC_SLATE_LEN: the nn.Module), the trainer's own forward
    (``score_block``: the step's kernels, dropout off, hipGraph replay) or the nn.Module (fp32 library GEMMs).  Every ``max(n, 1)``:
    an empty shard still enters the loss (its normaliser all-reduce is a collective) with one fully padded slate: value 0, count 0."""
    from . import _lib as LB
    if resident:                                                  # packed straight from the resident set: no padded features
        n = len(batch.ids)
        scorer = _val_scorer(scorers, trainer, -(-loader.batch_size // world), loader.slate_length)
        scorer.run_resident(batch.slates, batch.ids, batch.lengths)
        return _ValBatch(scorer.scores[:n], scorer.y, scorer.scores_raw[:max(n, 1)], scorer.y[:max(n, 1)], n, batch.global_slates, scorer)
    xb, yb, idx, n_glob, pre = _my_block(batch, loader, rank, world)
    n = int(xb.shape[0])
    if scorers is not None and int(xb.shape[1]) <= LB.MAX_METRIC_SLATE_LEN:
        scorer = _val_scorer(scorers, trainer, n, int(xb.shape[1]))
        scorer.run(xb, yb, idx, lengths=_host_lengths(batch, n, pre, world))
        return _ValBatch(scorer.scores[:n], yb, scorer.scores_raw[:max(n, 1)], scorer.y[:max(n, 1)], n, n_glob, scorer)
    own = trainer.score_block(xb, yb, idx, _host_lengths(batch, n, pre, world)) if trainer is not None and scorers is None else None
    if own is not None:
        return _ValBatch(own[0], yb, own[1], own[2], n, n_glob, None)
    if scorers is not None:
        last_run["val_scorer_reason"] = ("a slate length of %d is above LTRX_MAX_METRIC_SLATE_LEN = %d: module path"
                                         % (int(xb.shape[1]), LB.MAX_METRIC_SLATE_LEN))
    if ragged is not None:
        last_run["val_eval"] = {"loss": "padded", "metrics": "padded"}      # a batch no scorer could take
    if n == 0:
        xb, yb, idx = _pad_batch(xb, yb, idx, 1)
    mask = yb == PADDED_Y_VALUE
    out = model(xb, mask, idx)
    return _ValBatch((out if out.dim() == 2 else model.score(xb, mask, idx))[:n], yb, out, yb, n, n_glob, None)


def _cu_layout(packed, k, B):
    """layout arguments of a ragged loss / metric over the first ``k`` slates of ``FusedScorer.packed()`` (launch order: all B only)"""
    _, _, cu, order, max_len = packed
    return dict(cu_seqlens=cu[:k + 1], max_len=max(max_len, 1), slate_order=order if k == B else None)


def _evaluate(model, loss_func, dl, device, metrics, trainer=None, world=1, rank=0, scorers=None, ragged=None):
    """validation pass of train_utils.py:101-107: mean loss (weighted by batch size) and metric means, no autograd.  Which forward
    scores a batch: ``_score_batch``.  ``scorers`` (a dict, fit(val_scorer="packed")): the FusedScorers, one per slate length, kept
    across epochs; the batches come as ``id_batches`` when the loader is a packable DeviceLoader.
    ``ragged`` (a ``_ragged_plan``, fit(val_scorer="ragged")): for the batches a scorer ran, the loss and the metrics the plan names
    are computed from ``FusedScorer.packed()`` instead of the padded grid; same values (the ragged contract, include/ltrx.h).
    Sharded (``world`` > 1): every rank scores its block of each batch -- the training step's partition -- under
    ``shard_context(global batch)``, so its loss is its share of the reference's loss on the whole batch; one all-reduce
    at the end, and every rank returns the same numbers (scheduler and early stopping stay in step)."""
    from . import _lib as LB, sharding
    stats = _EpochStats(metrics, device)
    pf = dl if isinstance(dl, _Prefetcher) else _Prefetcher(dl, device)
    loader = pf.loader
    resident = (scorers is not None and getattr(loader, "packable", False) and getattr(loader, "world", 1) == world
                and loader.slate_length <= LB.MAX_METRIC_SLATE_LEN)
    with torch.no_grad():
        for batch in (loader.id_batches() if resident else pf):
            vb = _score_batch(batch, loader, resident, model, trainer, scorers, ragged, world, rank)
            n, pk = vb.n, vb.packed if ragged is not None else None
            rag_loss, rag_metrics = (ragged["loss"], ragged["metrics"]) if pk is not None else (None, ())
            # (an empty shard: one empty slate in the ragged loss, as the padded path's one padded slate, and no metric)
            packed = pk.packed() if rag_loss is not None or (rag_metrics and n > 0) else None
            if loss_func is None:                                     # (metrics only: the reference's compute_metrics pass)
                share = stats.tot.new_zeros(())
            else:
                fn, args, kw = ((rag_loss, packed[:2], _cu_layout(packed, max(n, 1), pk.B)) if rag_loss is not None else
                                (loss_func, (vb.out, vb.labels), {}))
                with sharding.shard_context(vb.n_glob) if world > 1 else contextlib.nullcontext():
                    share = fn(*args, **kw).detach().float()
            stats.add(share, vb.n_glob, n)
            if n > 0:
                for name, ats in metrics.items():
                    v = (getattr(RG, name)(packed[0], packed[1], ats=ats, **_cu_layout(packed, n, pk.B)) if name in rag_metrics else
                         getattr(EM, name)(vb.scores, vb.y[:n], ats=ats))
                    stats.add_metric(name, v.sum(0))
    loss_sum, n_slates, sums = stats.finish(world, zero_fill=True)
    n_all = max(float(n_slates), 1.0)
    return float(loss_sum) / n_all, {k: np.float32(v / n_all) for k, v in sums.items()}


def _assert_finite(trainer, loss, epoch, step):
    """the anomaly switch (main.py:89): raise on the first step whose loss, or what the engine's ``first_nonfinite`` scans, is not
    finite and name the first offending parameter tensor.  The step has already applied the update -- the run stops either way."""
    name, count = trainer.first_nonfinite()
    loss_ok = bool(torch.isfinite(loss.detach()).all().item())
    if name is not None or not loss_ok:
        raise FloatingPointError(
            "allrank_amd.fit (detect_anomaly / LTRX_CHECK_FINITE): step %d of epoch %d produced %s%s -- first offending parameter "
            "tensor: %s (%d non-finite %s element(s) in all).  Usual causes: non-finite input features, a learning rate that "
            "diverged, a slate with no valid item in a loss that divides by its normaliser."
            % (step, epoch, "a non-finite loss" if not loss_ok else "a finite loss", "" if name is None else " and non-finite values",
               name, count, trainer.scanned))


def fit(epochs, model, loss_func, optimizer, scheduler, train_dl, valid_dl, config, gradient_clipping_norm, early_stopping_patience,
        device, output_dir, tensorboard_output_path, use_fused=True, compact=None, gemm="split_bf16", train_metrics=None,
        check_finite=None, val_scorer=None, checkpoint_every=None, resume=None):
    """Same positional / keyword arguments as the reference ``fit``; ``use_fused`` / ``compact`` / ``gemm`` / ``train_metrics`` /
    ``check_finite`` are extensions (compact=None: variable-length execution when less than 80 % of the first batch's slots are valid
    items; compact="graph", or ALLRANK_AMD_COMPACT=graph under main.py (any other value raises): the variable-length step at bucketed
    row counts, captured and replayed per bucket -- FusedTrainer(compact="graph"), opt-in, never chosen by None; where it cannot
    apply (a sharded run, the slate-resident FC + ListNet step, stochastic NeuralNDCG) the job runs as under compact=True and
    ``last_run["compact_graph_reason"]`` says why; ``last_run["compact"]`` stays a bool and ``last_run["compact_graph"]`` =
    {"buckets": steps per row bucket, "captures", "replays", "eager_steps", "evictions"} (None when the mode is off); gemm: the arithmetic of the fused step, "split_bf16" = fp32-class parity arithmetic, "bf16" = the one-product throughput
    mode, see FusedTrainer; train_metrics: "fused" (default) = from the training forward, "reference" = the reference's second pass,
    train_utils.py:99; check_finite: None = ``config.detect_anomaly`` or LTRX_CHECK_FINITE=1, see the module docstring; val_scorer:
    "module" (default) = the validation batches of another slate length than the training step's run the nn.Module forward,
    "packed" = every validation batch runs the packed, captured forward-only scorer of the fused step (engine.FusedScorer; the
    environment variable ALLRANK_AMD_VAL_SCORER=packed does the same under main.py), "ragged" = "packed", and the loss and the
    ndcg / dcg / mrr metrics of those batches run on the packed rows as well (allrank_amd.ragged) -- the loss when
    ``ragged.form_of(loss_func)`` exists, anything else on the padded grid exactly as under "packed";
    ``last_run["val_scorer"]`` says which one ran, ``last_run["val_scorer_reason"]`` why the packed one could not, and
    ``last_run["val_eval"]`` = {"loss": "ragged" | "padded", "metrics": "ragged" | "padded"} what the "ragged" scorer evaluated on);
    checkpoint_every=k (or ALLRANK_AMD_CHECKPOINT_EVERY=k): after every k-th epoch, and after the last epoch the loop runs, the whole
    state of the run -- weights, optimizer moments and step count, the fused step's generator words, learning rate, scheduler,
    early stopping, the last metrics and every host generator -- replaces ``output_dir/checkpoint.pt`` atomically
    (allrank_amd.checkpoint; ``last_run["checkpoint"]`` = {"path", "every", "written"}, the written epochs' ``epoch_log`` entries gain
    "ckpt_s"); resume=path or "auto" (or ALLRANK_AMD_RESUME; "auto": ``output_dir/checkpoint.pt`` if it exists, else a fresh start)
    continues such a run at the epoch after the stored one, bit for bit where the uninterrupted run repeats itself bit for bit
    (``last_run["resume"]`` = {"path", "epoch"}); a file of another model, optimizer, loss or clipping norm raises ValueError, a file
    whose run had ended returns its stored result; both options raise NotImplementedError under a process group of several ranks)."""
    import torch.distributed as dist
    device = torch.device(device)
    world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
    checkpoint_every, resume = CK.options(checkpoint_every, resume)
    if world > 1 and (checkpoint_every is not None or resume is not None):
        raise NotImplementedError("allrank_amd.fit: checkpoint_every / resume under a process group of %d ranks -- per-rank generator "
                                  "state and the write barrier are not built; run without them" % world)
    if isinstance(model, torch.nn.DataParallel):
        # main.py:76-78 wrapped the model because several GPUs are visible.  The engine does not replicate inside one process: under a
        # process group every rank already holds its replica (allrank_amd.launch rebinds the wrapper away); without one, say so --
        # the whole (gpu_count x batch_size) batch of dataset_loading.py:240-241 is about to train on ONE device.
        n_vis = len(getattr(model, "device_ids", None) or [])
        model = model.module
        if world == 1:
            log.warning("allrank_amd.fit: the model arrived wrapped in nn.DataParallel over %d GPUs but no torch.distributed process "
                        "group is up -- training runs on %s ALONE, the other GPUs stay idle.  Start the job as "
                        "`python -m allrank_amd.launch --nproc %d -- <main.py arguments>` (one process per GPU, slate-sharded).",
                        n_vis, device, max(n_vis, 2))
    metrics = dict(config.metrics)
    val_metric = getattr(config, "val_metric", None)
    train_metrics_mode = (train_metrics or os.environ.get("ALLRANK_AMD_TRAIN_METRICS") or "fused").lower()
    if train_metrics_mode not in ("fused", "reference"):
        raise ValueError("train_metrics must be 'fused' or 'reference', got %r" % (train_metrics_mode,))
    val_scorer_mode = (val_scorer or os.environ.get("ALLRANK_AMD_VAL_SCORER") or "module").lower()
    if val_scorer_mode not in ("module", "packed", "ragged"):
        raise ValueError("val_scorer must be 'module', 'packed' or 'ragged', got %r" % (val_scorer_mode,))
    if check_finite is None:
        check_finite = bool(getattr(config, "detect_anomaly", False)) or os.environ.get("LTRX_CHECK_FINITE", "0") not in ("", "0")
    writer = _tensorboard(tensorboard_output_path) if tensorboard_output_path else None
    num_params = sum(p.numel() for p in model.parameters() if p.requires_grad)
    early_stop = _EarlyStop(early_stopping_patience)
    rank = dist.get_rank() if world > 1 else 0

    spec, reason = _fused_spec(model, loss_func, optimizer) if use_fused else (None, "use_fused=False")
    trainer, fused = None, False
    B_glob, L, valid_frac = _batch_shape(train_dl)
    lo, hi = shard_slates(B_glob, rank, world)
    compact = _compact_mode(compact)
    cg_reason = ""
    if spec is not None:
        if compact is None:
            compact = valid_frac < 0.8
        if compact == "graph" and world > 1:                      # (the trainer would refuse; the job keeps the fused step)
            compact, cg_reason = True, "slate-sharded run (%d ranks): the ranks' row buckets differ; compact=True" % world
        try:
            trainer = FusedTrainer(model, spec[0], spec[1], hi - lo, L, lr=spec[2], world_size=world, use_graph=True,
                                   gradient_clipping_norm=gradient_clipping_norm, compact=compact, gemm=gemm, **spec[3])
            fused = True
            optimizer._opt_called = True   # (torch's "scheduler.step() before optimizer.step()" check: in the fused run the
            #                                 optimizer object only carries the learning rate, its step() is never called)
            if compact == "graph" and not trainer.compact_graph:
                cg_reason = ("the slate-resident FC + ListNet step is taken: it reads the padded batch in place" if trainer.fcstep else
                             "stochastic NeuralNDCG reads the scores of padded slots: the step stays on the padded grid")
        except (NotImplementedError, KeyError) as e:
            reason = "FusedTrainer: %s" % (e,)
    if trainer is None:
        trainer = Trainer(model, loss_func, optimizer, gradient_clipping_norm, world, None)
    last_run.clear()
    last_run.update(engine="fused" if fused else "autograd", compact=bool(trainer.compact), reason=reason,
                    fcstep=trainer.fcstep, sampling=getattr(train_dl, "sampling", None),
                    compact_graph=_compact_graph_stats(trainer), compact_graph_reason=cg_reason)
    log.info("allrank_amd.fit: %s step%s", last_run["engine"], (" (" + reason + ")") if reason else "")
    normalizer = getattr(getattr(train_dl, "dataset", None), "normalizer", None)      # load_libsvm_dataset(normalize=...) hung it there
    if normalizer is not None:
        last_run["normalize"] = normalizer.report
    vs_reason = _packed_blocker(loss_func, fused, reason) if val_scorer_mode in ("packed", "ragged") else ""
    scorers = {} if val_scorer_mode in ("packed", "ragged") and not vs_reason else None
    last_run.update(val_scorer=val_scorer_mode if scorers is not None else "module", val_scorer_reason=vs_reason)
    rag_plan = _ragged_plan(loss_func, trainer, metrics) if val_scorer_mode == "ragged" and scorers is not None else None
    if rag_plan is not None:
        last_run["val_eval"] = {"loss": "ragged" if rag_plan["loss"] is not None else "padded",
                                "metrics": "ragged" if rag_plan["metrics"] else "padded"}
    if vs_reason:
        log.info("allrank_amd.fit: validation through the nn.Module forward (%s)", vs_reason)

    epoch, train_metrics, val_metrics = -1, {}, {}
    train_pf, valid_pf = _Prefetcher(train_dl, device), _Prefetcher(valid_dl, device)     # one per loader: stream and staging sets persist
    checked = world == 1
    last_run["epoch_log"] = []            # per epoch: wall seconds of the training / validation pass, slates and slots trained on
    n_steps = 0
    first_epoch, ckpt_path, rng_state = 0, os.path.join(output_dir, CK.FILE_NAME), None
    ckpt_meta = trainer.meta() if checkpoint_every is not None or resume is not None else None
    if checkpoint_every is not None:
        last_run["checkpoint"] = {"path": ckpt_path, "every": checkpoint_every, "written": 0}
    if resume == "auto" and not os.path.exists(ckpt_path):
        log.info("allrank_amd.fit: resume=auto and no %s: starting fresh", ckpt_path)
        resume = None
    if resume is not None:
        ck = CK.load(ckpt_path if resume == "auto" else resume)
        trainer.load_state_dict(ck["trainer"])                    # (checks compatibility before it touches anything)
        for g, lr in zip(optimizer.param_groups, ck["trainer"].get("lrs") or [ck["trainer"]["lr"]] * len(optimizer.param_groups)):
            g["lr"] = float(lr)
        if scheduler and ck["scheduler"] is not None:
            scheduler.load_state_dict(ck["scheduler"])
        early_stop.best_value, early_stop.best_epoch = ck["early_stop"]["best_value"], int(ck["early_stop"]["best_epoch"])
        epoch, n_steps = int(ck["epoch"]), int(ck["n_steps"])
        train_metrics, val_metrics = dict(ck["train_metrics"]), dict(ck["val_metrics"])
        first_epoch = epochs if ck["early_stop"]["stopped"] else epoch + 1
        rng_state = ck["rng"]
        last_run["resume"] = {"path": ckpt_path if resume == "auto" else resume, "epoch": epoch}
        log.info("allrank_amd.fit: resumed %s (epoch %d finished%s)", last_run["resume"]["path"], epoch,
                 "" if first_epoch < epochs else "; nothing left to train")
    if rng_state is not None and first_epoch < epochs:
        CK.restore_rng(rng_state, device)  # last: whatever building the job drew from the generators no longer matters
    for epoch in range(first_epoch, epochs):
        model.train()
        t_epoch = time.perf_counter()
        stats, slots = _EpochStats(metrics, device), 0
        for batch in train_pf:
            xb, yb, idx, real_glob, pre = _my_block(batch, train_dl, rank, world)
            if not checked:
                _check_same_batch(batch[0], batch[1], world, pre)
                checked = True
            real = int(xb.shape[0])
            loss = trainer.step_block(xb, yb, idx, real_glob, _host_lengths(batch, real, pre, world))
            n_steps += 1
            if check_finite:
                _assert_finite(trainer, loss, epoch, n_steps)
            stats.add(loss.detach().float(), real_glob, real)         # (sharded: this rank's share of the global-batch loss)
            slots += real * int(yb.shape[1])
            if train_metrics_mode == "fused":
                for name, ats in metrics.items():
                    # (a rank whose shard of a short last batch is empty contributes zeros -- every rank keeps the same stats layout)
                    stats.add_metric(name, getattr(EM, name)(trainer.scores[:real], trainer.y_cur[:real], ats=ats).sum(0) if real > 0
                                     else torch.zeros(len(ats), device=device))
        loss_sum, n_slates, sums = stats.finish(world, zero_fill=False)
        t_train = time.perf_counter() - t_epoch
        last_run["compact_graph"] = _compact_graph_stats(trainer)
        n_all = max(n_slates, 1.0)
        train_loss = float(loss_sum) / n_all
        train_metrics = {k: float(v) / n_all for k, v in sums.items()}
        if train_metrics_mode == "reference":
            # train_utils.py:99: compute_metrics(config.metrics, model, train_dl, device) -- one more pass over train_dl per metric
            # name (:46-54), with the end-of-epoch weights, the model still in train() mode
            train_metrics = {}
            for name, ats in metrics.items():
                _, one = _evaluate(model, None, train_pf, device, {name: ats}, trainer, world, rank)
                train_metrics.update({k: float(v) for k, v in one.items()})
        else:
            _burn(train_dl, len(metrics))                          # the generator draws of the passes not made (module docstring)

        model.eval()
        t_val = time.perf_counter()
        val_loss, val_metrics = _evaluate(model, loss_func, valid_pf, device, metrics, trainer, world, rank, scorers, rag_plan)
        _burn(valid_dl, len(metrics))                              # train_utils.py:107 iterates valid_dl once more per metric name
        last_run["epoch_log"].append({"train_s": t_train, "val_s": time.perf_counter() - t_val, "slates": int(n_slates),
                                      "slots": int(slots), "val_loss": val_loss})

        if writer is not None:
            tb = {("train", "loss"): train_loss, ("val", "loss"): val_loss, ("train", "lr"): optimizer.param_groups[0]["lr"]}
            tb.update({("train", k): v for k, v in train_metrics.items()})
            tb.update({("val", k): v for k, v in val_metrics.items()})
            writer.save_to_tensorboard(tb, epoch)
        log.info("Epoch : %d Train loss: %s Val loss: %s %s %s", epoch, train_loss, val_loss,
                 " ".join("Train %s %s" % kv for kv in train_metrics.items()), " ".join("Val %s %s" % kv for kv in val_metrics.items()))

        current = val_metrics.get(val_metric)
        if scheduler:                                              # train_utils.py:117-122
            if type(scheduler) is torch.optim.lr_scheduler.ReduceLROnPlateau:
                scheduler.step(val_metrics[val_metric])
            else:
                scheduler.step()
            trainer.set_lr(float(optimizer.param_groups[0]["lr"]))  # the scheduler edits optimizer.param_groups; the engine follows
        early_stop.step(current, epoch)
        if checkpoint_every is not None and ((epoch + 1) % checkpoint_every == 0 or epoch == epochs - 1 or early_stop.stop_training(epoch)):
            t_ck = time.perf_counter()
            CK.save(ckpt_path, {
                "epoch": epoch, "n_steps": n_steps, "engine": last_run["engine"],
                "trainer": trainer.state_dict(),
                "scheduler": scheduler.state_dict() if scheduler else None,
                "early_stop": {"best_value": early_stop.best_value, "best_epoch": early_stop.best_epoch,
                               "stopped": bool(early_stop.stop_training(epoch))},
                "train_metrics": train_metrics, "val_metrics": val_metrics, "rng": CK.capture_rng(device), "meta": ckpt_meta})
            last_run["checkpoint"]["written"] += 1
            last_run["epoch_log"][-1]["ckpt_s"] = time.perf_counter() - t_ck
        if early_stop.stop_training(epoch):
            log.info("early stopping at epoch %d since %s didn't improve from epoch no %d. Best value %s, current value %s",
                     epoch, val_metric, early_stop.best_epoch, early_stop.best_value, current)
            break

    if rank == 0:
        torch.save({k: v.detach().clone() for k, v in model.state_dict().items()}, os.path.join(output_dir, "model.pkl"))
        if normalizer is not None:                       # what the model's inputs went through: needed to score raw features later
            normalizer.save(os.path.join(output_dir, NORMALIZATION_FILE))
    if writer is not None:
        writer.close_all_writers()
    return make_result(epoch, train_metrics, val_metrics, num_params)
