"""Training-step driver for the hot path: the body of ``loss_batch`` (allrank/training/train_utils.py:18-29) without
its per-step host syncs, on device-resident data, optionally slate-sharded across ranks.

    mask = (yb == -1); loss = loss_func(model(xb, mask, indices), yb); loss.backward(); [clip]; opt.step(); opt.zero_grad()

Differences from the reference driver (all outside the arithmetic): no ``loss.item()`` per step (the loss stays on
the device; call ``.item()`` when you want it), gradients live in one flat buffer (allrank_amd.parallel), and under
``world_size > 1`` the loss is normalised by the global batch and gradients are summed over RCCL.
"""
import collections
import contextlib
import ctypes
import functools
import gc
import logging
import warnings

import torch
from torch.nn.utils import clip_grad_norm_

from . import kernels as KN, parallel, rows as RW, sharding
from .rows import row_bucket, _stage_host, _Stager  # noqa: F401  (their home is allrank_amd/rows.py; imported from here too)

PADDED_Y_VALUE = -1

# The step's operands, made once by FusedTrainer.__init__ (the flat buffers are never rebound, so a view or an address stays right):
#   Param  one per nn.Parameter, ``FusedTrainer.params`` in flat-buffer order: its name, the parameter, its offset, and the views of
#          flat_p / flat_g shaped like it;
#   Lin    one per projection (nn.Linear; q, k, v of a layer are ONE [3d, d] projection): weight, bias and their gradients, ``wT`` the
#          contiguous transposed copy inside flat_t (or None), ``w_img`` / ``wT_img`` the addresses of the pre-split images of w / wT
#          (None without images), and for the first FC layer over padded input rows ``w_pad`` / ``w_pad_img``: the zero-padded copy
#          the forward multiplies instead of w;
#   Norm   one per LayerNorm: scale, shift, their gradients and eps.
Param = collections.namedtuple("Param", "name p off w g")
Norm = collections.namedtuple("Norm", "a b ga gb eps")


class Lin(object):
    __slots__ = ("w", "b", "gw", "gb", "off", "wT", "w_img", "wT_img", "w_pad", "w_pad_img")

    def __init__(self, w, b, gw, gb, off):
        self.w, self.b, self.gw, self.gb, self.off = w, b, gw, gb, off
        self.wT = self.w_img = self.wT_img = self.w_pad = self.w_pad_img = None


class Trainer(object):
    """The autograd engine.  What the epoch loop (fit.py) needs, it and FusedTrainer offer under the same names: ``step_block``,
    ``score_block``, ``first_nonfinite`` / ``scanned``, ``set_lr``, ``meta`` / ``state_dict`` / ``load_state_dict``, ``compact`` ..."""
    compact = compact_graph = fcstep = False      # the variable-length layouts and the slate-resident step are FusedTrainer's
    scanned = "weight"                            # what first_nonfinite() reads

    def __init__(self, model, loss_func, optimizer, gradient_clipping_norm=None, world_size=1, group=None):
        self.model, self.loss_func, self.opt = model, loss_func, optimizer
        self.clip, self.world, self.group = gradient_clipping_norm, world_size, group
        self.flat = parallel.FlatGradients(model.parameters(), group)
        self._meta = None                             # meta(), made once

    def step_block(self, xb, yb, indices, global_batch, lengths=None):
        """``step`` on this rank's block of a global batch, short or empty; leaves ``scores[:n]`` / ``y_cur[:n]`` (as FusedTrainer's)"""
        if xb.shape[0] == 0:
            # (sharded: this rank's block of a short last batch is empty -- the step still has to run, its gradient all-reduce
            #  is a collective: one fully padded slate, i.e. zero loss and zero gradients.  Found by the 2-rank autograd job of
            #  tests/dist_fit_worker.py in round 5: the nn.Module forward raised on 0 rows while the peer sat in the all-reduce.)
            xb, yb, indices = pad_batch(xb, yb, indices, 1)
        loss = self.step(xb, yb, indices, global_batch=global_batch)
        self.scores, self.y_cur = self.last_scores, yb
        return loss

    def score_block(self, xb, yb, indices, lengths=None):
        return None                               # no forward of its own: validation runs the nn.Module (FusedTrainer.score_block)

    def first_nonfinite(self):
        """as FusedTrainer's, over the WEIGHTS the last step left: ``flat.zero()`` has run, the gradients are gone"""
        bad = [(n, int((~torch.isfinite(p.detach())).sum().item())) for n, p in self.model.named_parameters()]
        return next((n for n, k in bad if k), None), sum(k for _, k in bad)

    def set_lr(self, lr):
        """nothing to do: the optimizer object a scheduler edits is the one that steps (FusedTrainer: a launch argument)"""

    # ---- checkpointing: FusedTrainer's three members for the nn.Module and the torch optimizer, in the schema of checkpoint.py -----
    def meta(self):
        """what ``checkpoint.check_compatible`` compares, as FusedTrainer's; made once: its lr is the job's first (never compared)"""
        from . import checkpoint as CK
        if self._meta is None:
            g, kind, f = self.opt.param_groups[0], CK.neutral_kind(self.opt), self.loss_func
            hyper = CK.group_hyper(g) if kind is None else CK.hyper(kind, g["lr"], g.get("betas"), g.get("eps"), g.get("weight_decay", 0.0),
                                                                    g.get("momentum", 0.0), g.get("nesterov", False))
            if isinstance(f, functools.partial):
                name, args = getattr(f.func, "__name__", repr(f.func)), dict(f.keywords or {})
                if f.args:
                    args["*"] = list(f.args)
            else:
                name, args = getattr(f, "__name__", type(f).__name__), {}
            self._meta = CK.make_meta(list(self.model.named_parameters()), kind or type(self.opt).__name__, hyper, name, args, self.clip)
        return self._meta

    def state_dict(self):
        """a checkpoint's "trainer" entry: the module's state_dict, the optimizer's state in the neutral schema (raw outside it)"""
        from . import checkpoint as CK
        return {"params": {k: v.detach().cpu() for k, v in self.model.state_dict().items()},
                "optimizer": CK.to_neutral(self.opt, self.model.named_parameters()),
                "lr": float(self.opt.param_groups[0]["lr"]), "lrs": [float(g["lr"]) for g in self.opt.param_groups], "meta": self.meta()}

    def load_state_dict(self, state):
        """a checkpoint's "trainer" entry into the live job, in place; compatibility first (ValueError, nothing touched).  Either
        engine loads either engine's entry -- only a raw torch optimizer state is tied to this engine and its own class."""
        from . import checkpoint as CK
        CK.check_compatible(state["meta"], self.meta())
        raw = "torch_optimizer" in state["optimizer"]
        if raw != (CK.neutral_kind(self.opt) is None) or (raw and state["optimizer"]["kind"] != type(self.opt).__name__):
            raise ValueError("checkpoint: the stored optimizer state (%s, %s) does not fit the live %s"
                             % (state["optimizer"]["kind"], "raw" if raw else "neutral", type(self.opt).__name__))
        for n, p in self.model.named_parameters():
            if n not in state["params"] or tuple(state["params"][n].shape) != tuple(p.shape):
                raise ValueError("checkpoint: parameter %s: no tensor of shape %s in the checkpoint" % (n, tuple(p.shape)))
        with torch.no_grad():
            for k, v in self.model.state_dict().items():
                if k in state["params"] and tuple(state["params"][k].shape) == tuple(v.shape):
                    v.copy_(state["params"][k])
        CK.from_neutral(self.opt, self.model.named_parameters(), state["optimizer"])

    def step(self, xb, yb, indices=None, global_batch=None):
        """one training step on this rank's slates; returns the (device) loss tensor -- this rank's share of the
        global loss when sharded."""
        self.flat.check()         # .grad must still alias the flat buffer (an external zero_grad(set_to_none=True) detaches it)
        mask = (yb == PADDED_Y_VALUE)
        gb = global_batch if global_batch is not None else xb.shape[0] * self.world
        with sharding.shard_context(gb, self.group) if self.world > 1 else contextlib.nullcontext():
            out = self.model(xb, mask, indices)
            loss = self.loss_func(out, yb)
        # scores of THIS forward (model.py:82-92: d_output > 1 sums the last axis), for train metrics without a second pass
        self.last_scores = out.detach() if out.dim() == 2 else out.detach().sum(-1)
        loss.backward()
        if self.world > 1:
            self.flat.all_reduce()
        if self.clip:
            clip_grad_norm_(self.model.parameters(), self.clip)
        self.opt.step()
        self.flat.zero()          # == opt.zero_grad(set_to_none=False): grads stay views of the flat buffer
        return loss


# ------------------------------------------------------------------------------------------------------------------
# shared by FusedTrainer and FusedScorer: the forward-buffer plan and the forward-graph cache (the row layouts, their batch stager
# and their movers: allrank_amd/rows.py)
# ------------------------------------------------------------------------------------------------------------------
def input_row_plan(F, H, M, gemm, has_input_norm, pad_input):
    """How the rows the first FC projection reads are laid out: ``(stride, K, large)`` for ``F`` input features, a first FC width
    ``H``, ``M`` rows per step, the trainer's ``gemm`` mode, an ``input_norm`` or none, and its ``pad_input`` option.
      stride: floats per row of the operand buffer (the features are its first F columns, the rest stays zero);
      K:      columns the projection contracts over -- the ``[:, :K]`` view of the buffer against W_0 zero-padded to [H, K];
      large:  rows of 256 floats and K a multiple of the GEMM's 32-column step, so that the first layer runs the large-tile forward and
              weight-gradient kernels (a large batch into a 256-multiple width, no input_norm, the bf16-MFMA arithmetic).
    ``stride == K == F`` is the dense form: no padded buffer, W_0 itself.  F % 4 != 0 -- a feature count the data set dictates
    (46, 45, 137) -- never has it: ltrx_gemm_nt takes K and row strides in multiples of 4 floats, so stride and K are at least F
    rounded up to 4.  Pure: no GPU, no library."""
    large = bool(pad_input and not has_input_norm and gemm in ("split_bf16", "bf16") and F % 256 != 0 and F <= 1024
                 and H % 256 == 0 and M >= 2048)
    if large:
        return (F + 255) // 256 * 256, (F + 31) // 32 * 32, True
    F4 = (F + 3) // 4 * 4
    return F4, F4, False


def _alloc_forward(owner, t, rows, B, L, saved, layout):
    """Create on ``owner`` the buffer set that ``FusedTrainer._forward`` of trainer ``t`` runs over (``B`` slates of ``L`` items, up to
    ``rows`` rows), every buffer zero-initialised.  The only place that makes forward buffers, and the list of what ``_forward`` reads
    from a buffer set ``bs``:
      B, L, layout ("grid", "index" or "cu": allrank_amd/rows.py), saved; rows (of THIS pass: kept current by the owner, not here)
      mask [B, L] u8 key padding (None in the scorer's form: packed rows are all valid keys)
      cu [B+1], order [B] (views of the owner's ``_stager`` tensor), idx [rows] packed row -> grid slot: the packed layouts, else None
      x_in [rows, F]; x_norm [rows, F], mean_in, rstd_in (input_norm only); fc_out[i].  With t._x_pad (``input_row_plan``: the
      large-tile form, or F % 4 != 0) the rows the first projection reads -- x_in, or x_norm under input_norm (x_in is then dense:
      no GEMM reads it) -- are the ``[:, :F]`` view of a buffer with rows of t._x_stride floats (x_in_buf / x_norm_buf), and x_in_k
      is its ``[:, :t._x_k]`` view, the GEMM operand.  INVARIANT: the columns from F on are zero at allocation and nothing writes
      them again -- every staging kernel, the strided input LayerNorm included, writes F columns per row -- so the K - F surplus
      columns of the contraction multiply zeros, whatever the pad columns of w0_pad hold (zeros too)
      idx_rows (i64 rank of every row, -1 = none) and x_pe: positional encoding only
      layers[i]: lin_qkv, lin_o, lin_ff1, lin_ff2, norm0, norm1, p_*, s_* (the trainer's operand records and dropout sites of the
      layer: t._layer_ops[i]; its own dicts later hold rbits), xsum0 (the residual stream entering layer i > 0), xn0, mean0, rstd0, qkv, o, lse, x1, xn1, mean1,
      rstd1, r, and q, k, v (the column views of qkv that the attention launches read);  xsum_f, xf, mean_f, rstd_f (the final norm; xf
      is None where t.norm_head holds: the fused final norm + score head keeps the normalised rows in registers);  scores_c (packed layouts only), scores_raw [B, L(, n_out)], scores [B, L]
    ``saved=True``, the trainer's form: the backward reads the activations, so every layer has its own.  ``saved=False``, the scorer's:
    ONE activation set serves every layer -- the residual stream ping-pongs between two buffers (a layer's input is dead once its
    out-projection has added it: xsum0 of layer i = ping[i % 2], xsum_f = ping[N % 2], x_pe = ping[0], which layer 0 reads while
    writing ping[1]) and one LayerNorm output / statistics set serves LN0, LN1 and the final norm (each is consumed before the next is
    written)."""
    dev, d, no, F0 = t.dev, t.d, t.n_out, t.fc_sizes[0]

    def z(*shape):
        return torch.zeros(shape, dtype=torch.float32, device=dev)

    def ln():
        return z(rows, d), z(rows), z(rows)

    def acts(ln0, ln1):
        qkv = z(rows, 3 * d)
        q, k, v = KN.thirds(qkv)
        return dict(xn0=ln0[0], mean0=ln0[1], rstd0=ln0[2], xn1=ln1[0], mean1=ln1[1], rstd1=ln1[2], qkv=qkv, q=q, k=k, v=v, o=z(rows, d),
                    lse=z(B, t.h, L), x1=z(rows, d), r=z(rows, t.dff))

    if layout not in ("grid", "index", "cu"):
        raise ValueError("layout must be grid, index or cu, got %r" % (layout,))
    owner.B, owner.L, owner.layout, owner.saved = B, L, layout, bool(saved)
    compact = layout != "grid"
    owner.mask = torch.zeros((B, L), dtype=torch.uint8, device=dev) if saved else None
    owner._stager = _Stager(dev, B, with_ids=not saved) if compact else None
    owner.cu, owner.order = (owner._stager.cu, owner._stager.order) if compact else (None, None)
    owner.idx = torch.full((rows,), 0 if saved else -1, dtype=torch.int32, device=dev) if compact else None
    if t._x_pad:
        op = z(rows, t._x_stride)                             # the first projection's operand rows
        owner.x_in_k = op[:, :t._x_k]
        if t.in_norm is None:
            owner.x_in_buf, owner.x_in = op, op[:, :F0]
        else:
            owner.x_in, owner.x_norm_buf, owner.x_norm = z(rows, F0), op, op[:, :F0]
    else:
        owner.x_in = z(rows, F0)
        if t.in_norm is not None:
            owner.x_norm = z(rows, F0)
    if t.in_norm is not None:
        owner.mean_in, owner.rstd_in = z(rows), z(rows)
    owner.fc_out = [z(rows, s) for s in t.fc_sizes[1:]]
    if t.pos is not None:
        owner.idx_rows = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    owner.layers = []
    if t.N and saved:
        for i, ops in enumerate(t._layer_ops):
            owner.layers.append(dict(ops, xsum0=z(rows, d) if i else None, **acts(ln(), ln())))
        owner.xsum_f = z(rows, d)
        owner.xf, owner.mean_f, owner.rstd_f = (None, z(rows), z(rows)) if t.norm_head else ln()
    elif t.N:
        ping, one = [z(rows, d), z(rows, d)], ln()
        shared = acts(one, one)
        for i, ops in enumerate(t._layer_ops):
            owner.layers.append(dict(ops, xsum0=ping[i % 2], **shared))
        owner.xsum_f = ping[t.N % 2]
        owner.xf, owner.mean_f, owner.rstd_f = (None,) + one[1:] if t.norm_head else one
    if t.pos is not None:
        owner.x_pe = ping[0] if (t.N and not saved) else z(rows, d)
    if compact:
        owner.scores_c = z(rows) if no == 1 else z(rows, no)
    owner.scores_raw = z(B, L) if no == 1 else z(B, L, no)    # what the loss sees (model.forward)
    owner.scores = owner.scores_raw if no == 1 else z(B, L)   # model.score (sum over the output units)


@contextlib.contextmanager
def _collector_at_rest():
    """Python's cyclic collector stays out of a hipGraph recording.  A trainer or scorer that has been dropped is cyclic garbage (its
    graph cache refers back to it), and collecting it destroys its hipGraphs and returns their memory pool: runtime calls that a
    thread must not make while it records.  So what is dead is collected first, as torch.cuda.graph does on entry, and the collector
    rests until the recording is closed."""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


class _GraphLRU(object):
    """The capture-and-replay rule of every hipGraph the engine records (training step, ``score()``, the scorer's row buckets): two
    eager warm-up visits stay outside any capture (lazy module loads, kernel attributes, workspaces), then a key is captured --
    a list of ``(hipGraph, host action | None)`` segments, recording only -- and replayed: each graph, then its action.  The captures
    form an LRU of ``max_graphs`` keys (``graphs``: least recently used first; emptying it is how captures are dropped); a new key
    beyond that first evicts the oldest (``evictions`` counts them, ``on_evict(key)`` hears of each)."""

    def __init__(self, max_graphs, capture=None, warm="key", on_evict=lambda key: None, new_pool=None):
        # (nothing of torch.cuda is touched before the default ``capture`` or ``new_pool`` runs: a fake of either drives this on a CPU)
        self.graphs, self._visits = collections.OrderedDict(), collections.Counter()
        self.max_graphs, self.evictions, self._on_evict = int(max_graphs), 0, on_evict
        # capture(fn): records ``fn`` into ``self.pool`` and returns the segments; default: one torch.cuda.graph
        self._capture = capture or self._record
        # warm: what the two warm-up visits are counted over --
        #   "key":   each key.  The forward users: a new row bucket can select kernels that were never launched, and a first launch
        #            (module load, kernel attributes) must stay outside a capture.
        #   "cache": the whole cache, once.  The training step: a new batch divisor changes only a by-value scalar of launches that
        #            have all been made before, so every later key is captured on its first visit.
        #   a function of the key: the part of the key it returns.  The variable-length training step, keyed (batch divisor,
        #            collectives on?, row bucket), counts over the row bucket: both reasons above, one per part of its key.
        self._slot = warm if callable(warm) else {"key": lambda key: key, "cache": lambda key: None}[warm]
        # new_pool(): the memory-pool handle the captures share (None: every capture gets a private pool of the default kind).  A
        # pool whose graphs are all gone cannot be captured into again, so capture_now starts a fresh one whenever ``graphs`` is
        # empty -- however it got empty: a caller's ``graphs.clear()`` (set_lr, bench.py), an eviction with max_graphs = 1.
        self._new_pool, self.pool = new_pool, None

    def _record(self, fn):
        g = torch.cuda.CUDAGraph()
        with _collector_at_rest(), torch.cuda.graph(g, pool=self.pool):
            fn()
        return [(g, None)]

    def capture_now(self, key, fn=None):
        """record ``key`` unless it is live -- nothing executes; False (and nothing recorded) while its warm-up is not over"""
        if key in self.graphs:
            return True
        if self._visits[self._slot(key)] < 2:
            return False
        while len(self.graphs) >= self.max_graphs:
            self.evictions += 1
            self._on_evict(self.graphs.popitem(last=False)[0])
        if not self.graphs and self._new_pool is not None:
            self.pool = self._new_pool()
        self.graphs[key] = self._capture(fn)                  # (a capture that raises leaves no entry)
        return True

    def run(self, key, fn):
        """run, capture and replay, or replay ``fn`` for ``key``; returns "eager", "capture" or "replay" """
        mode = "replay" if key in self.graphs else "capture"
        if not self.capture_now(key, fn):
            self._visits[self._slot(key)] += 1
            fn()
            return "eager"
        self.graphs.move_to_end(key)
        for g, after in self.graphs[key]:                     # (capture only records: the replay executes this visit)
            g.replay()
            if after is not None:
                after()
        return mode


def pad_batch(xb, yb, idx, B):
    """top a short batch up to ``B`` slates with fully padded ones (features 0, label -1, index -1: no loss, no gradient)"""
    n = B - xb.shape[0]
    if n <= 0:
        return xb, yb, idx
    return (torch.cat([xb, xb.new_zeros((n,) + tuple(xb.shape[1:]))]),
            torch.cat([yb, yb.new_full((n, yb.shape[1]), float(PADDED_Y_VALUE))]),
            torch.cat([idx, idx.new_full((n, idx.shape[1]), -1)]))


# ------------------------------------------------------------------------------------------------------------------
# FusedTrainer: the same training step, written out explicitly (no autograd) on preallocated buffers
# ------------------------------------------------------------------------------------------------------------------
class FusedTrainer(object):
    """One training step of train_utils.py:18-29 as a fixed launch sequence on persistent HBM buffers:

        FC -> N x [LN -> QKV GEMM -> fused attention -> out GEMM(+res) -> LN -> FFN GEMMs(+ReLU, +res)] -> LN
           -> score head -> fused listwise loss (value + d/dscores) -> hand-written backward -> [RCCL all-reduce]
           -> fused Adam over ONE flat parameter buffer.

    * parameters / gradients / Adam moments are single flat fp32 buffers; the nn.Module's parameters are re-pointed
      at views of the flat buffer, so ``model.state_dict()`` / ``model.score()`` always see the trained weights, and
      the Q,K,V projection weights of a layer sit adjacently => ONE [3d, d] GEMM feeds the attention kernel in place.
    * every gradient is written exactly once per step straight into the flat gradient buffer (GEMM ``out=`` views):
      no zero_grad pass, no accumulation kernels, one collective for multi-GPU.
    * every launch of the sequence is a libltrx kernel: the dense projections are the split-bf16 MFMA GEMMs
      (ltrx_gemm_nt / ltrx_gemm_tn; ``gemm="hipblaslt"`` swaps in torch.mm/addmm as a comparison arithmetic).
    * the whole sequence is captured in a hipGraph after warm-up (``use_graph=True``) -- at 64 slates/GPU the step is
      ~100 launches of 10-300 us, so launch latency matters.  The variable-length step (``compact=True``)
      runs eagerly: its row count changes per batch.  ``compact="graph"`` (opt-in) rounds that count up the scorer's row ladder and
      captures one step per row bucket (see ``__init__``; faster or not: profiles/compact_graph.md).
    * dropout (every shipped transformer config trains with 0.1-0.4) is counter-based: a mask element is a hash of
      (site seed ^ per-step device word, element index), generated inside the producing kernel's epilogue (GEMM bias+
      ReLU+dropout, the residual sum in the epilogue of the projection that closes a sublayer, the attention probabilities)
      and REGENERATED in the backward
      -- no mask tensors, and a replayed hipGraph draws fresh masks because the step word lives in device memory.
    * every loss of allrank_amd.losses with every argument, ``stochastic=True`` of neuralNDCG / neuralNDCG_transposed included: its
      Gumbel noise is one more site of the same generator (FusedLoss; the last draw stays in ``self.loss.gumbel``).  Such a job
      runs on the padded grid (``compact`` is dropped: the batch-wide minimum reads the scores of padded slots) and on one
      rank (sharded: NotImplementedError -- a global minimum and tie count would take two more collectives per step).
    Supported model family: FCModel (optional input_norm = nn.LayerNorm, activation None / ReLU, or Sigmoid / Tanh without FC
    dropout) -> optional encoder with
    optional fixed / learned positional encoding (positional.py:15-77) -> OutputLayer(any d_output, activation None / Sigmoid /
    Tanh; d_output > 1 feeds the ``ordinal`` loss, ``scores`` is then the sum over the output units, model.py:119-128).
    Other FC / output activations raise NotImplementedError (use ``Trainer``).
    The input feature count is free: where it is no multiple of 4 (46, 45, 137) the first projection reads rows padded to the next one
    against a zero-padded copy of W_0 (``input_row_plan``).  The widths the model chooses -- FC widths, d_ff, the head width
    d_model / h -- must be multiples of 4 (head width <= 128): anything else raises NotImplementedError here, naming the width.
    """

    def __init__(self, model, loss_name, loss_args, B, L, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, world_size=1, group=None,
                 optimizer="Adam", weight_decay=0.0, momentum=0.0, nesterov=False,
                 use_graph=True, gemm="split_bf16", dropout=True, seed=None, gradient_clipping_norm=None, compact=False,
                 weight_images=True, fc_step=True, group_wgrad=True, relu_bits=True, pad_input=True, force_dist=False,
                 _norm_head=True, ln_in_wgrad=True):
        """gemm: "split_bf16" -- libltrx fp32-accurate GEMMs on the bf16 MFMA (3 products), "split_bf16_strict" (6
        products), "hipblaslt" (torch.mm/addmm, exact-fp32 library GEMMs), or "bf16" -- the THROUGHPUT mode: one bf16
        product per contraction in the dense projections AND in attention (fp32 storage, accumulation, LayerNorm, softmax,
        loss and Adam; about 2^-9 relative error per product, outside the 1e-5 parity contract -- bench.py reports it
        on its own line with its measured loss error).  dropout=False trains with every
        nn.Dropout of the model disabled; seed keys the dropout masks (default: torch.initial_seed(), nothing is drawn from the global generator);
        gradient_clipping_norm: clip_grad_norm_ of train_utils.py:24-25 (the coefficient stays on the device).
        compact=True: variable-length execution -- the valid items of each padded batch (dataset.py:28-38) are packed into
        consecutive rows, every row-wise kernel runs over the packed rows only, attention reads per-slate extents from
        cu_seqlens, and scores / d loss/d scores move between the packed rows and the padded [B, L] grid the loss kernels
        work on.  Same loss and gradients as the padded step (padded rows carry no gradient and are masked as keys); the
        row count changes per batch, so this mode runs eagerly (no hipGraph).
        The buffer set's ``self.layout`` (allrank_amd/rows.py) names the three forms: "grid" (compact=False: the padded B * L rows),
        "index" (compact=True: rows packed through a host-sized index, ceil32(n) of them) and "cu" (compact="graph", and every
        FusedScorer: rows packed from cu_seqlens in device memory, ``row_bucket`` of them); ``self.compact`` / ``self.compact_graph``
        are read off it, and staging, ``_forward`` and ``_body`` decide by it alone.
        compact="graph" (opt-in; ``self.compact`` is True, ``self.compact_graph`` says so): the same packed step at BUCKETED row
        counts, captured and replayed per bucket.  The row count is ``row_bucket(n, ceil32(B * L))``, the scorer's ladder (the
        buffers hold its largest rung), and a captured step is keyed (batch divisor, collectives on?, rows); the two eager
        warm-up visits are counted per row bucket (a new bucket can pick GEMM tiles and LayerNorm launch shapes that were never
        launched), a new divisor inside a warmed bucket is captured on its first visit, the LRU holds 8 captures.  Nothing
        inside the sequence depends on a host copy of the valid-row count: packing, unpacking and the zeroing of the
        alignment rows the attention kernels leave out read it from cu_seqlens in device memory (ltrx_gather_rows_cu,
        ltrx_scatter_rows_cu, ltrx_zero_rows_cu).  Staging stays outside the graph and, with host ``lengths``, without a host
        sync.  ``use_graph=False`` runs the identical launch sequence eagerly; ``self.last_mode`` is "eager", "capture" or
        "replay" for the last step.  Costs and limits: rows n .. rows-1 are alignment rows (zero input, no slate, no gradient;
        every buffer a later kernel reads there is written for them in the same step, so they are a function of the weights
        alone) -- up to 31 rows below 256, up to 1/8 of the bucket above, where compact=True runs at most 31; the valid items
        must come first in every slate (how dataset.py pads; without ``lengths`` the one counting sync also checks it and a
        batch with interior padding raises ValueError -- that stays a compact=True capability); slate-sharded trainers raise
        NotImplementedError (ranks see different row counts, hence different keys); whether it is faster than compact=True:
        profiles/compact_graph.md.
        optimizer: "Adam" (betas, eps, weight_decay = L2 term), "AdamW" (decoupled weight decay) or "SGD" (momentum, nesterov,
        weight_decay; dampening 0) -- torch.optim's update rules (main.py:82) in one flat-buffer kernel.
        weight_images=False: the GEMMs split the weight operand on the fly in every tile instead of reading the per-step pre-split
        images (same results bit for bit; kept for A/B measurements).
        fc_step=True: a model that is FCModel([H]) -> OutputLayer(H, 1) with the listNet loss (BASELINE configs[1]) trains through
        the slate-resident step of ltrx_fc_listnet_step -- forward, loss, backward and Adam in two launches that read the batch
        from HBM once, straight from the caller's tensors (no staging copy, no hipGraph needed); False keeps the GEMM launch
        sequence for A/B runs; "collapse" (opt-in, FC activation None only): the linear scorer's two layers evaluated as ONE
        matrix-vector product per slate with the exact rank-1 gradients (ltrx_fc_linear_listnet_step: fp32 FMAs, the slate in registers,
        HBM-bound).  ``self.fcstep`` tells which one is active (False / True / "collapse").
        group_wgrad=True: the four weight gradients of an encoder layer run as one ltrx_gemm_tn_group launch (4x fewer partial slabs
        to write and reduce); False = one ltrx_gemm_tn per projection (A/B runs).
        relu_bits=True: the feed-forward ReLU(+dropout) mask travels from the forward GEMM to the input-gradient GEMM as one bit per
        element (ltrx_gemm_nt acts 4 / 5) instead of being re-read from the saved fp32 activation; same results bit for bit.
        pad_input=True: the static input buffer keeps the features in rows padded to 256 floats so that the first FC layer (F = 136 is
        no multiple of the GEMM's 32-column step) runs the large-tile forward and weight-gradient kernels; False = dense rows (A/B) -- or,
        for a feature count that is no multiple of 4, rows padded to the next one, which the GEMM entries need (``input_row_plan``).
        (Round 6: the two opt-in NEGATIVE RESULTS of round 5 -- ``overlap_wgrad`` (fork / join of the weight-gradient launches on a
        second stream: 1-2 % slower, profiles/r05_wgrad_overlap_ab.md) and ``act_images`` (activations as pre-split operand images:
        VALU -6 ... -28 % in the consumers, cycles unchanged, step -1 %, profiles/r05_act_images_ab.md) -- no longer live in this class;
        tools/lab/patches/r06_engine_overlap_wgrad_act_images.patch re-adds them; the image-form kernel entry points that act_images drove
        (ltrx_gemm_nt_img, ltrx_gemm_tn_group_img, ltrx_layernorm_fwd_image) have left the library too: the patch's act_images half
        needs the library of commit 68005e3.)
        force_dist=True: see ``self.sharded`` below.
        _norm_head=True: the encoder's final norm and the d_output == 1 score head run as one kernel each way (ltrx_norm_head_fwd /
        ltrx_norm_head_bwd_partial / ltrx_norm_head_wgrad: the normalised rows and their gradient never reach HBM) where ``self.norm_head`` says so; False keeps
        ltrx_layernorm_* + ltrx_score_head_* (A/B runs, tests: the same bits everywhere).
        ln_in_wgrad=True (with group_wgrad): the first-sublayer LayerNorm backward of an encoder layer runs INSIDE the layer's grouped
        weight-gradient launch, on the CUs that launch leaves without a workgroup (ltrx_gemm_tn_group_ln: 48 tiles x 5 splits = 240 of 256),
        instead of as a launch of its own behind it; the residual-stream gradient then rotates over three buffers, because that
        LayerNorm backward may no longer write into the buffer the weight gradient is reading.  Same bits; False = the two launches."""
        from . import _lib as LB
        from .losses import FusedLoss
        self.LB = LB
        self.lib = LB.lib()
        if gemm not in ("split_bf16", "split_bf16_strict", "hipblaslt", "bf16"):
            raise ValueError("gemm must be split_bf16, split_bf16_strict, hipblaslt or bf16")
        self.gemm = gemm
        self.weight_images = bool(weight_images)
        self.group_wgrad = bool(group_wgrad) and gemm != "split_bf16_strict"     # (the strict arithmetic has no large-tile kernel)
        self.ln_in_wgrad = bool(ln_in_wgrad) and self.group_wgrad and gemm != "hipblaslt"
        self.ln_side_log = []                 # side workgroups the most recent ltrx_gemm_tn_group_ln calls used (0: the two-launch path)
        self._wg_pending = []
        self.wgrad_group_log = []             # (problems, grouped kernel ran?) of the most recent _wgrad_flush calls
        self._red_pending = []                # (src ptr, partial rows, row stride, columns, dst ptr) entries of the next _reduce_flush
        self._ln_slot = 0
        self._prec = {"split_bf16_strict": 1, "bf16": 2}.get(gemm, 0)        # precision code of ltrx_gemm_nt / ltrx_gemm_tn
        # attention arithmetic of THIS trainer, passed with every ltrx_mha_fwd / ltrx_mha_bwd call (the library keeps no mode):
        # 1 = three bf16 products (fp32-class, parity), 2 = one product (the "bf16" throughput mode)
        self._mha_mode = 2 if gemm == "bf16" else 1
        self.model = model
        self.B, self.L, self.M = B, L, B * L
        self.lr, self.betas, self.eps = lr, betas, eps
        if optimizer not in ("Adam", "AdamW", "SGD"):
            raise NotImplementedError("FusedTrainer: optimizer %r (Adam, AdamW and SGD are fused)" % (optimizer,))
        self.optimizer, self.weight_decay = optimizer, float(weight_decay)
        self.momentum, self.nesterov = float(momentum), bool(nesterov)
        self.world, self.group = world_size, group
        # the step takes its SHARDED form (global divisor through shard_context, bucketed all-reduce of the flat gradient behind the
        # backward, normaliser all-reduces, hipGraph segments cut at every collective) when there is more than one rank -- or when
        # ``force_dist`` asks for it on a one-rank group: the whole collective path, RCCL included, on the one GPU a build box has
        # (bench.py --force-dist, tests/test_gpu_rccl.py).  Needs an initialised process group.
        self.sharded = bool(world_size > 1 or force_dist)
        stoch = loss_name in ("neuralNDCG", "neuralNDCG_transposed") and bool((loss_args or {}).get("stochastic"))
        if stoch and self.sharded:
            raise NotImplementedError("FusedTrainer: stochastic NeuralNDCG under slate sharding -- the batch-wide minimum of the scores and "
                                      "its tie count (loss_utils.py:102) would take two more collectives per step")
        self.clip = float(gradient_clipping_norm) if gradient_clipping_norm else None
        seed = self._read_model(model, dropout, seed)
        # final norm + score head fused: an encoder, one output unit, a register-resident width (D = 256 NV <= 1024), and the deferred
        # reduction of the LayerNorm partials (_reduce_flush), whose sums the two-kernel path's (a_2, b_2) gradients have there
        self.norm_head = bool(_norm_head and self.N > 0 and self.n_out == 1 and self.d % 256 == 0 and self.d <= 1024
                              and self.group_wgrad and gemm != "hipblaslt")
        # slate-resident FC + ListNet step (csrc/ltrx_fcstep.hip): eligibility.  It reads the padded batch in place and masks padded
        # items itself, so a request for variable-length execution is moot for such a job (and would only route it to the slower
        # GEMM launch sequence): compact is dropped.
        fc_ok = bool(
            fc_step and self.N == 0 and self.nfc == 1 and self.in_norm is None and self.pos is None and self.fc_act in (0, 1)
            and self.p_fc == 0.0 and self.n_out == 1 and self.out_act == 0 and loss_name == "listNet"
            and gemm == "split_bf16" and optimizer in ("Adam", "AdamW")
            and self.lib.ltrx_fc_listnet_supported(L, self.fc_sizes[0], self.fc_sizes[1]))
        if not fc_ok:                                         # (before the module's parameters are re-pointed: a refusal leaves it untouched)
            self._check_widths()
        if isinstance(compact, str) and compact != "graph":
            raise ValueError("compact must be False, True or \"graph\", got %r" % (compact,))
        # compact="graph": the packed step at bucketed row counts, captured per bucket -- not for the two jobs that drop compact below
        graph_rows = compact == "graph" and not fc_ok and not stoch
        if graph_rows and self.sharded:
            raise NotImplementedError("FusedTrainer(compact=\"graph\") under slate sharding: the ranks' blocks of a batch hold different "
                                      "numbers of valid items, so their row buckets -- the keys of the captured steps -- differ, and "
                                      "agreeing on captured-versus-eager per step across ranks is not built; use compact=True")
        offs = self._layout_parameters(dropout)
        if fc_ok:
            if compact or not use_graph:
                logging.getLogger("allrank_amd.engine").info(
                    "FusedTrainer: the slate-resident FC + ListNet step is taken (two launches per step, the padded batch read in place): "
                    "compact=%s / use_graph=%s do not apply to it; scores / labels of the last step alias the caller's tensors until the "
                    "next step()", compact, use_graph)
            compact = False
        # stochastic NeuralNDCG takes its minimum over the padded slots' scores too (loss_utils.py:102): the packed step computes no
        # score there (it leaves 0), so the step stays on the padded grid
        if stoch and compact:
            logging.getLogger("allrank_amd.engine").info(
                "FusedTrainer: stochastic NeuralNDCG reads the scores of padded slots (batch-wide minimum): compact=%s does not apply "
                "to it", compact)
            compact = False
        # forward buffers (the trainer is its own buffer set).  Input rows are padded to a multiple of 256 floats where the first FC
        # layer can then run the large-tile GEMMs: the forward projection contracts over F rounded up to the kernel's 32-column step
        # against a row-padded copy of W_0 (refreshed with the weight images), the weight gradient reads the padded rows as tiles.
        # A feature count that is no multiple of 4 (MQ2007 / MQ2008: 46, OHSUMED: 45) takes the same route whatever the batch: the
        # GEMMs address rows and K in multiples of 4 floats, so the rows are padded to the next one (input_row_plan).
        F0 = self.fc_sizes[0]
        self._x_stride, self._x_k, self._x_large = input_row_plan(F0, self.fc_sizes[1], self.M, gemm, self.in_norm is not None, pad_input)
        self._x_pad = (self._x_stride, self._x_k) != (F0, F0)
        # rows every row buffer holds: the padded grid -- or, for the bucketed rows of compact="graph", the largest rung of the
        # scorer's ladder (every slot valid), as FusedScorer sizes its set
        layout = "cu" if graph_rows else "index" if compact else "grid"
        self.cap = (self.M + 31) // 32 * 32 if layout == "cu" else self.M
        _alloc_forward(self, self, self.cap, B, L, saved=True, layout=layout)
        self.rows = B * L                                                     # rows the row-wise kernels run over
        self.n_valid = B * L
        self.y_in = torch.zeros((B, L), dtype=torch.float32, device=self.dev)
        self._alloc_backward(relu_bits)
        self._fused_images = False
        if self.gemm != "hipblaslt":
            self._init_weight_images()
        self.loss = FusedLoss(loss_name, B, L, self.dev, **(loss_args or {}))
        self._loss_args = dict(loss_args or {})               # as bound by the caller (meta(): what a checkpoint is compared on)
        if self.loss.stochastic:                             # Gumbel noise: a site of the step's generator, re-keyed by drop_step
            self.loss.set_noise_key(self._site_seeds()[1], self.drop_step)
        if (self.n_out > 1) != (loss_name == "ordinal") or (loss_name == "ordinal" and int(loss_args["n"]) != self.n_out):
            raise NotImplementedError("FusedTrainer: d_output > 1 goes with the ordinal loss of the same n (and only with it)")
        # ListMLE: the reference draws torch.randperm(L) on every call (listMLE.py:17).  shuffle_ties=True (default) does
        # the same with a device generator; tests that compare with the oracle set shuffle_ties=False and an explicit
        # permutation via ``trainer.loss.set_perm``.
        self.shuffle_ties = True
        self._perm_gen = torch.Generator(device=self.dev)
        self._perm_gen.manual_seed(int(seed) & 0x7FFFFFFF)
        self.use_graph = use_graph and (not compact or self.compact_graph)
        self.last_mode = None                                 # "eager" / "capture" / "replay" of the last step()
        self.mode_counts = collections.Counter()              # ... of every step() so far
        self.bucket_counts = collections.Counter()            # compact="graph": steps per row bucket
        self._fwd_graphs = _GraphLRU(1)                       # score(): one key, captured into the default pool
        self.probe = None                                     # list collecting (start, end) events of the FFN1 GEMM (eager steps only)
        self.probe_wgrad = None                               # ... of the grouped weight-gradient launch (bench.py, eager steps only)
        # captured steps: {(batch divisor, collectives on?): [(hipGraph segment, collective to launch after it | None), ...]}
        # The batch divisor is a by-value launch argument of the loss kernels (include/ltrx.h: `batch_divisor`), i.e. a captured
        # step keeps the divisor it was captured with.  Captured steps are therefore keyed by the divisor: the short last batch of
        # an epoch (DataLoader drop_last=False, dataset_loading.py:245; it arrives topped up with padded slates and global_batch =
        # its real slate count) gets its own capture.  The captures form an LRU of ``max_graphs`` (4) entries: a fifth distinct
        # divisor evicts the least recently used one (and says so once) instead of silently running eagerly.
        # compact="graph": the key grows by the row bucket -- (batch divisor, collectives on?, rows) -- the warm-up visits are counted
        # per bucket (_GraphLRU: a function of the key), and the LRU holds 8 captures, as the scorer's
        self.max_graphs = 8 if self.compact_graph else 4
        self._step_graphs = _GraphLRU(self.max_graphs, capture=lambda fn: self._capture(),
                                      warm=(lambda key: key[2]) if self.compact_graph else "cache", on_evict=self._warn_evicted,
                                      new_pool=torch.cuda.graph_pool_handle)
        self._graphs = self._step_graphs.graphs               # (live mapping: least recently used first)
        self.capture_fallback = None                          # why the step is not captured: the capture error after which a sharded
        #                                                       run fell back to eager steps, or ensure_captured()'s "not warmed up"
        self._seg_break = None                                # set while capturing: ends the current segment (see _capture)
        self._cap_stream = None
        self._wver = [r.p._version for r in self.params]
        self._images_stale = False
        self.y_cur = self.y_in                                # labels of the last step() (the caller's tensor in the fcstep path)
        self.keep_fc_out = False                              # tests: also write the FC activations to fc_out[0]
        self.keep_loss_grad = False                           # tests: also write d loss / d scores to self.loss.grad (4 B per item)
        self.fcstep = fc_ok
        if self.fcstep and fc_step == "collapse" and self.fc_act == 0:
            self.fcstep = "collapse"
        if self.fcstep:
            self._init_fc_step(offs)

    # the public facts about variable-length execution, read off the buffer set's layout (allrank_amd/rows.py)
    compact = property(lambda self: self.layout != "grid", doc="the step runs over the packed valid rows")
    compact_graph = property(lambda self: self.layout == "cu", doc="... packed from cu_seqlens at bucketed row counts, captured per bucket")

    # ---- the named steps of __init__ ---------------------------------------------------------------------------
    def _read_model(self, model, dropout, seed):
        """the model family check and what the step reads off the nn.Module (sizes, activations, dropout); returns the resolved seed"""
        import torch.nn as nn
        from .model import FCModel, Encoder, LTRModel, LearnedPositionalEncoding
        if not isinstance(model, LTRModel) or not isinstance(model.input_layer, FCModel):
            raise NotImplementedError("FusedTrainer needs an allrank_amd LTRModel with an FCModel input block")
        fc = model.input_layer
        self.in_norm = None if isinstance(fc.input_norm, nn.Identity) else fc.input_norm      # nn.LayerNorm (model.py:27)
        self.p_fc = float(fc.dropout.p) if dropout else 0.0
        if seed is None:
            # derived from the seed torch's global generator was given (main.py:36: torch.manual_seed(42)) WITHOUT drawing from it: the
            # loaders' shuffle order comes from that generator, and a draw here would shift every epoch's batches away from the
            # reference's (round 6: the trajectory fixtures of tests/golden/make_golden_trajectory.py)
            seed = int(torch.initial_seed() & 0x7FFFFFFF)
        self._seed = (int(seed) * 0x9E3779B1 + 0x7F4A7C15 * (1 + self._rank(self.group, self.world))) & 0xFFFFFFFF
        if isinstance(fc.activation, nn.Identity):
            self.fc_act = 0
        elif isinstance(fc.activation, nn.ReLU):
            self.fc_act = 1
        elif isinstance(fc.activation, (nn.Sigmoid, nn.Tanh)) and self.p_fc == 0.0:
            # (model.py:28-29 resolves any torch.nn name; Sigmoid / Tanh run as an elementwise pass after the GEMM whose derivative is
            #  taken from the stored output -- with dropout after them the stored output no longer determines it: autograd Trainer)
            self.fc_act = 3 if isinstance(fc.activation, nn.Sigmoid) else 4
        else:
            raise NotImplementedError("FusedTrainer: FC activation %r%s" % (fc.activation, " with dropout" if self.p_fc else ""))
        enc = model.encoder if isinstance(model.encoder, Encoder) else None
        self.pos = enc.position if (enc is not None and enc.position is not None) else None
        self.pos_learned = isinstance(self.pos, LearnedPositionalEncoding)
        if self.pos is not None:
            if self.pos_learned:
                self.pos_pad = int(self.pos.pe.padding_idx)
            else:
                self.pos_pad = int(self.pos.padding_idx)
        out = model.output_layer
        self.n_out = int(out.d_output)                # > 1: ordinal configs (model.py:111-128: forward [B, L, d_output], score = sum)
        if isinstance(out.activation, nn.Identity):
            self.out_act = 0
        elif isinstance(out.activation, nn.Sigmoid):
            self.out_act = 1
        elif isinstance(out.activation, nn.Tanh):
            self.out_act = 2
        else:
            raise NotImplementedError("FusedTrainer: output activation %r" % (out.activation,))
        self.dev = next(model.parameters()).device
        self.enc = enc
        self.nfc = len(fc.layers)
        self.fc_sizes = [fc.layers[0].in_features] + [l.out_features for l in fc.layers]
        self.d = self.fc_sizes[-1]
        self.N = len(enc.layers) if enc is not None else 0
        if enc is not None:
            l0 = enc.layers[0]
            self.h = l0.self_attn.h
            self.dff = l0.feed_forward.w_1.out_features
            self.ln_eps = enc.norm.eps
        return seed

    def _check_widths(self):
        """What the GEMM launch sequence cannot run is refused HERE, with the width named, so that a caller with another engine to turn
        to (fit(): the autograd Trainer) takes it before the first batch instead of dying in it.  The input feature count is free
        (input_row_plan); every width the model itself chooses is a row length of an activation the GEMMs, the LayerNorms and the
        attention kernels address in 16-byte pieces: a multiple of 4, and a head width ltrx_mha_fwd takes."""
        for i, s in enumerate(self.fc_sizes[1:]):
            if s % 4:
                raise NotImplementedError("FusedTrainer: FC layer %d is %d wide -- the fused step takes hidden widths that are multiples "
                                          "of 4 (the input feature count is free)" % (i, s))
        if self.N:
            if self.dff % 4:
                raise NotImplementedError("FusedTrainer: feed-forward width d_ff = %d is no multiple of 4" % self.dff)
            if self.d % self.h or not self.lib.ltrx_mha_head_width_supported(self.d // self.h):
                raise NotImplementedError("FusedTrainer: head width d_model / h = %d / %d -- the attention kernels take head widths that "
                                          "are multiples of 4 up to 128" % (self.d, self.h))
        if self.in_norm is not None and self.fc_sizes[0] < 2:
            raise NotImplementedError("FusedTrainer: input_norm over %d feature (ltrx_layernorm_bwd needs at least 2 columns)" % self.fc_sizes[0])

    def _site_seeds(self):
        """the seeds, under the current ``_seed``, of the dropout sites of every encoder layer (one dict per layer, keyed as the layer
        dicts are) and of the stochastic loss's noise"""
        return ([dict(s_att=self._site(4 * i), s_ff=self._site(4 * i + 1), s_s0=self._site(4 * i + 2), s_s1=self._site(4 * i + 3))
                 for i in range(self.N)], self._site(2000))

    def _layout_parameters(self, dropout):
        """the flat parameter / gradient / moment buffers (16-byte aligned segments; q,k,v weights and biases adjacent) with the module's
        parameters re-pointed at them, the gradient buckets, and the operand records of the step: ``params`` (one Param per parameter, flat
        order), ``norm_in``, ``fc``, ``pos_table`` / ``pos_g``, per encoder layer the four Lin, two Norm and the dropout sites in
        ``_layer_ops`` (_alloc_forward adds the activations: ``layers``), ``norm_f`` and ``head``; returns the segment offsets"""
        model, fc, enc, out, dev = self.model, self.model.input_layer, self.enc, self.model.output_layer, self.dev
        order = []
        if self.in_norm is not None:
            order += [self.in_norm.weight, self.in_norm.bias]
        for lyr in fc.layers:
            order += [lyr.weight, lyr.bias]
        if self.pos_learned:
            order += [self.pos.pe.weight]
        if enc is not None:
            for lay in enc.layers:
                lin = lay.self_attn.linears
                order += [lin[0].weight, lin[1].weight, lin[2].weight, lin[0].bias, lin[1].bias, lin[2].bias,
                          lin[3].weight, lin[3].bias, lay.feed_forward.w_1.weight, lay.feed_forward.w_1.bias,
                          lay.feed_forward.w_2.weight, lay.feed_forward.w_2.bias,
                          lay.sublayer[0].norm.a_2, lay.sublayer[0].norm.b_2, lay.sublayer[1].norm.a_2, lay.sublayer[1].norm.b_2]
            order += [enc.norm.a_2, enc.norm.b_2]
        order += [out.w_1.weight, out.w_1.bias]
        named = list(model.named_parameters())                # (the order state_dict() and meta() keep)
        assert len(order) == len(named)
        offs, n = [], 0
        for p in order:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4
        self.nflat = n
        self.flat_p = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step_count = torch.zeros(1, dtype=torch.float32, device=dev)
        self.clip_scale = torch.ones(1, dtype=torch.float32, device=dev)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.ws_clip = KN.clip_workspace(self.lib, n, self.flat_g)
        self.drop_step = torch.zeros(1, dtype=torch.int32, device=dev)       # u32 word folded into every dropout seed
        self._works = []
        self.comm_enabled = True      # bench.py measures the exposed part of the collective by switching it off
        # the kernels address the flat buffers through the views of these records, never through p.data / p.grad: an external
        # zero_grad(set_to_none=True) or .to() cannot redirect the step (step() re-attaches the module's views)
        self.params = []
        with torch.no_grad():
            for p, o in zip(order, offs):
                view = self.flat_p[o:o + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                p.grad = self.flat_g[o:o + p.numel()].view_as(p)
                self.params.append(Param(next(name for name, q in named if q is p), p, o, view, p.grad))
        by_name = {r.name: r for r in self.params}
        self._params_named = [by_name[name] for name, _ in named]
        # the projections and norms, taken off the records in flat order
        rec, d = iter(self.params), self.d

        def lin():
            w, b = next(rec), next(rec)
            return Lin(w.w, b.w, w.g, b.g, w.off)

        def lin_qkv():                                        # q, k, v of a layer: adjacent segments read as one [3d, d] | [3d] projection
            w, _, _, b, _, _ = [next(rec) for _ in range(6)]
            return Lin(self.flat_p[w.off:w.off + 3 * d * d].view(3 * d, d), self.flat_p[b.off:b.off + 3 * d],
                       self.flat_g[w.off:w.off + 3 * d * d].view(3 * d, d), self.flat_g[b.off:b.off + 3 * d], w.off)

        def norm(eps):
            a, b = next(rec), next(rec)
            return Norm(a.w, b.w, a.g, b.g, eps)

        self.norm_in = norm(self.in_norm.eps) if self.in_norm is not None else None
        self.fc = [lin() for _ in fc.layers]
        # the positional table (transformer.py:51-52) and, for a learned one, its gradient
        self.pos_table, self.pos_g = next(rec)[3:] if self.pos_learned else (self.pos.pe if self.pos is not None else None, None)
        sites = self._site_seeds()[0]
        self._layer_ops = []
        for i in range(self.N):
            lay = enc.layers[i]
            self._layer_ops.append(dict(
                lin_qkv=lin_qkv(), lin_o=lin(), lin_ff1=lin(), lin_ff2=lin(), norm0=norm(self.ln_eps), norm1=norm(self.ln_eps),
                # dropout sites (transformer.py:105,155,227): probabilities and seeds
                p_att=float(lay.self_attn.dropout.p) if dropout else 0.0,
                p_ff=float(lay.feed_forward.dropout.p) if dropout else 0.0,
                p_s0=float(lay.sublayer[0].dropout.p) if dropout else 0.0,
                p_s1=float(lay.sublayer[1].dropout.p) if dropout else 0.0, **sites[i]))
        self.norm_f = norm(self.ln_eps) if enc is not None else None
        self.head = lin()
        self.layers = self._layer_ops                         # (until _alloc_forward gives every layer its activations)
        # gradient buckets for the multi-GPU all-reduce, in the order the backward completes them: the tail of the flat
        # buffer (last encoder layer + final norm + head) first, then one bucket per earlier layer, the FC stack last
        self._buckets = []
        prev_hi = n
        for ops in reversed(self._layer_ops):
            self._buckets.append((ops["lin_qkv"].off, prev_hi))
            prev_hi = ops["lin_qkv"].off
        self._buckets.append((0, prev_hi))
        # (no active dropout site -> no mask counter to advance: one launch less per step)
        self._any_dropout = bool(self.p_fc or any(st[k] for st in self.layers for k in ("p_att", "p_ff", "p_s0", "p_s1")))
        return offs

    def _alloc_backward(self, relu_bits):
        """gradient buffers and kernel workspaces of the backward (what _body and its helpers use beyond the forward buffer set)"""
        B, L, M, d, dev, compact, gemm = self.B, self.L, self.cap, self.d, self.dev, self.compact, self.gemm   # (M: rows per buffer)
        f32 = dict(dtype=torch.float32, device=dev)
        if self.in_norm is not None:
            F_ = self.fc_sizes[0]
            self.d_in = torch.zeros((M, F_), **f32)
            self.ws_ln_in = KN.layernorm_bwd_workspace(self.lib, M, F_, self.d_in)
        if relu_bits and self.N and self.dff % 256 == 0 and d % 32 == 0 and gemm not in ("hipblaslt", "split_bf16_strict"):
            # one bit per feed-forward activation (written by the forward GEMM, read by the input-gradient GEMM instead of r)
            for st in self.layers:
                st["rbits"] = torch.zeros(((M + 255) // 256) * (self.dff // 256) * 8192, dtype=torch.uint8, device=dev)
        if self.N:
            self.d_r = torch.zeros((M, self.dff), **f32)
            self.dqkv = torch.zeros((M, 3 * d), **f32)
            self.dq, self.dk, self.dv = KN.thirds(self.dqkv)    # (the views the attention backward writes through)
            self.d_o = torch.zeros((M, d), **f32)
            self.tmp_d = torch.zeros((M, d), **f32)
            self.d_br = torch.zeros((M, d), **f32)            # gradient of a dropped residual branch (ds * keep)
            self.ws_ln = KN.layernorm_bwd_workspace(self.lib, M, d, self.d_o)
            # deferred parameter-gradient partials of up to three LayerNorm backwards per encoder layer (_reduce_flush)
            self.ws_ln_g = [self.ws_ln] + [torch.empty_like(self.ws_ln) for _ in range(2)]
            self.ws_mha = KN.mha_bwd_workspace(self.lib, B, L, self.h, d // self.h, self._mha_mode, self.d_o)
        no = self.n_out
        if compact:
            self.dsc_c = torch.zeros(M if no == 1 else (M, no), **f32)
        if no > 1:
            npad = (no + 3) // 4 * 4
            self.dz_pad = torch.zeros((M, npad), **f32)        # d loss / d pre-activation, K padded to a multiple of 4 for the dgrad GEMM
            self.woutT_pad = torch.zeros((d, npad), **f32)     # W_out^T zero-padded the same way (refreshed after every optimizer step)
            self.head.wT = self.woutT_pad                      # (outside flat_t: no image)
            self.zb = torch.zeros(no, **f32)
        self.d_a = torch.zeros((M, d), **f32)                 # gradient w.r.t. the residual stream (ping)
        self.d_b = torch.zeros((M, d), **f32)                 # (pong)
        if self.N and self.ln_in_wgrad:                       # a third one: see the layer loop of _step_body
            self.d_c = torch.zeros((M, d), **f32)
        maxn = max([3 * d, self.dff if self.N else 0] + self.fc_sizes[1:])
        self.ws_col = KN.colsum_workspace(self.lib, M, maxn, self.d_a)
        self.ws_head = KN.score_head_bwd_workspace(self.lib, M, d, self.d_a)
        self.fc_dgrad = [torch.zeros((M, s), **f32) for s in self.fc_sizes[1:-1]]
        if self.gemm != "hipblaslt":
            nb = 0
            shapes = [(s1, s0) for s0, s1 in zip(self.fc_sizes[:-1], self.fc_sizes[1:])]
            if self.N:
                shapes += [(3 * d, d), (d, d), (self.dff, d), (d, self.dff)]
            if self.n_out > 1:
                shapes += [(self.n_out, d)]
            for (npp, kpp) in shapes:
                nb = max(nb, self.lib.ltrx_gemm_tn_workspace_bytes(M, npp, kpp))
            if self.N and self.group_wgrad:                       # the four projections of a layer in one launch (_wgrad_flush)
                # ... or, when both sublayer dropouts are on (the dropout buffer d_br is reused between the branches), as two groups of
                # two: fewer tiles per group -> more row splits per problem -> possibly MORE workspace than the group of four.  The
                # buffer covers every composition the step issues, in issue order
                w2, w1, wo, wq = (d, self.dff), (self.dff, d), (d, d), (3 * d, d)
                comps = [[w2, w1, wo, wq]]
                if any(st["p_s0"] and st["p_s1"] for st in self.layers):
                    comps += [[w2, w1], [wo, wq]]
                for comp in comps:
                    npa = (ctypes.c_int * len(comp))(*[c[0] for c in comp])
                    kpa = (ctypes.c_int * len(comp))(*[c[1] for c in comp])
                    nb = max(nb, self.lib.ltrx_gemm_tn_group_workspace_bytes(len(comp), M, npa, kpa))
            self.ws_tn = torch.empty(max(nb, 64), dtype=torch.uint8, device=dev)

    def _init_weight_images(self):
        """transposed weight copies for the input-gradient GEMMs (one flat buffer, one descriptor table, refreshed after every optimizer
        step by ONE batched transpose launch) and the pre-split images of the weights and of the copies; every Lin record learns its
        ``wT`` and, with ``weight_images``, the addresses of its images"""
        dev = self.dev
        f32 = dict(dtype=torch.float32, device=dev)
        if self._x_pad:                                           # the zero-padded copy [H, K] of W_0 the padded input rows multiply
            self.w0_pad = self.fc[0].w_pad = torch.zeros((self.fc_sizes[1], self.x_in_k.shape[1]), **f32)
            self.w0_pad_i = torch.zeros_like(self.w0_pad)
        # the table's order: the FC weights an input gradient is taken through (all but the first, which has one only under input_norm),
        # then per layer out, ff1, ff2, qkv
        lins = self.fc if self.in_norm is not None else self.fc[1:]
        for st in self.layers:
            lins = lins + [st["lin_o"], st["lin_ff1"], st["lin_ff2"], st["lin_qkv"]]
        tot = sum((l.w.numel() + 3) // 4 * 4 for l in lins)
        self.flat_t = torch.zeros(max(tot, 4), **f32)
        desc, tstart, o = [], [0], 0
        for l in lins:
            r, c = l.w.shape
            l.wT = self.flat_t[o:o + r * c].view(c, r)
            desc += [l.off, o, r, c]
            tstart.append(tstart[-1] + ((r + 31) // 32) * ((c + 31) // 32))
            o += (r * c + 3) // 4 * 4
        self._tdesc = torch.tensor(desc if desc else [0, 0, 0, 0], dtype=torch.int64, device=dev)
        self._tstart = torch.tensor(tstart, dtype=torch.int32, device=dev)
        self._tn, self._ttiles = len(lins), tstart[-1]
        # pre-split bf16 hi / lo IMAGES of the weights and of their transposes (same offsets as flat_p / flat_t): what the
        # large-tile NT GEMMs stage as operand B without splitting it again in every tile (ltrx_split_image, include/ltrx.h)
        self.flat_pi = torch.empty_like(self.flat_p)
        self.flat_ti = torch.zeros_like(self.flat_t)
        if self.weight_images:
            def image(view, base, img):                           # where ``img`` holds the image of ``view``, a piece of ``base``
                return ctypes.c_void_p(img.data_ptr() + view.data_ptr() - base.data_ptr())

            for l in self.fc + [self.head] + [st[k] for st in self.layers for k in ("lin_qkv", "lin_o", "lin_ff1", "lin_ff2")]:
                l.w_img = image(l.w, self.flat_p, self.flat_pi)
            for l in lins:
                l.wT_img = image(l.wT, self.flat_t, self.flat_ti)
            if self._x_pad:
                self.fc[0].w_pad_img = image(self.w0_pad, self.w0_pad, self.w0_pad_i)
        # one-launch refresh (ltrx_weight_images) when every transposed matrix keeps image groups of 4 inside a row
        self._fused_images = self.nflat % 4 == 0 and all(l.w.shape[0] % 4 == 0 for l in lins)
        self._refresh_transposes()

    def _init_fc_step(self, offs):
        """the slate-resident FC + ListNet step: its workspace and the parameter offsets its launch takes"""
        B, L = self.B, self.L
        F_, H_ = self.fc_sizes[0], self.fc_sizes[1]
        H4 = (H_ + 3) // 4 * 4
        offs_fc = (0, H_ * F_, H_ * F_ + H4, H_ * F_ + 2 * H4)
        assert tuple(offs) == offs_fc and self.nflat == offs_fc[3] + 4, (offs, self.nflat)
        self._fc_ws = KN.fc_listnet_workspace(self.lib, B, L, F_, H_, self.nflat, self.flat_p)
        if self.fcstep == "collapse":
            self._fc_ws = KN.fc_linear_listnet_workspace(self.lib, B, F_, self.flat_p)
        self._fc_offs = offs_fc

    # ---- thin launch helpers -----------------------------------------------------------------------------------
    def _st(self):
        return self.LB.launch_stream(self.dev)

    @staticmethod
    def _rank(group, world_size):
        if world_size <= 1:
            return 0
        import torch.distributed as dist
        return dist.get_rank(group)

    def _site(self, k):
        """seed of site k of the step's generator (one per nn.Dropout instance of the model; 2000: the stochastic loss's noise)"""
        x = (self._seed ^ ((k + 1) * 0x85EBCA6B)) & 0xFFFFFFFF
        x = ((x ^ (x >> 16)) * 0x7FEB352D) & 0xFFFFFFFF
        x = ((x ^ (x >> 15)) * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    def _ln_fwd(self, x, res, nm, xsum, y, mean, rstd, p=0.0, seed=0, rows=None):
        """y = LN(x + drop_p(res)) of the Norm ``nm``; xsum = x + drop_p(res)   (over ``rows`` rows, default the step's)"""
        KN.layernorm_fwd(self.lib, self._st(), x, res, nm.a, nm.b, self.rows if rows is None else rows, nm.eps, xsum, y, mean, rstd, p, seed,
                         self.drop_step)

    def _drop_apply(self, src, dst, p, seed):
        """dst = src * keep-mask/(1-p) of the site (the backward of a dropped branch)"""
        KN.dropout_apply(self.lib, self._st(), src, self.rows, p, seed, self.drop_step, dst)

    def _branch_grad(self, ds, p, seed):
        if p == 0.0:
            return ds
        self._drop_apply(ds, self.d_br, p, seed)
        return self.d_br

    def _ln_partial_slot(self):
        """the next free workspace for deferred (da, db) partial rows of a LayerNorm backward, or None: no deferred reduction in this
        configuration, or the layer has used its slots (the reduction then runs at once)"""
        if self.group_wgrad and self.gemm != "hipblaslt" and self._ln_slot < len(self.ws_ln_g):
            self._ln_slot += 1
            return self.ws_ln_g[self._ln_slot - 1]
        return None

    def _ln_partials_queue(self, buf, nrows, da, db):
        """``nrows`` partial rows [da(d) | db(d)] in ``buf`` join the layer's one reducing launch (_reduce_flush)"""
        self._red_pending.append((buf.data_ptr(), nrows, 2 * self.d, self.d, da.data_ptr()))
        self._red_pending.append((buf.data_ptr() + 4 * self.d, nrows, 2 * self.d, self.d, db.data_ptr()))

    def _ln_bwd(self, dy, xsum, nm, mean, rstd, dres, dx):
        buf = self._ln_partial_slot()
        if buf is not None:                                       # dx now, the parameter gradients with the layer's reductions
            nrows = KN.layernorm_bwd_partial(self.lib, self._st(), dy, xsum, nm.a, mean, rstd, dres, self.rows, nm.eps, dx, buf)
            self._ln_partials_queue(buf, nrows, nm.ga, nm.gb)
            return
        KN.layernorm_bwd(self.lib, self._st(), dy, xsum, nm.a, mean, rstd, dres, self.rows, nm.eps, dx, nm.ga, nm.gb, self.ws_ln)

    def _colsum(self, a, out):
        KN.colsum(self.lib, self._st(), a, self.rows, out, self.ws_col)

    def _relu_bwd(self, dr, r, p=0.0):
        """dr *= (r > 0) / (1 - p): backward of dropout(relu(z)) given the stored post-dropout activation r"""
        KN.relu_bwd(self.lib, self._st(), dr, r, self.rows, 1.0 / (1.0 - p))

    def saved_activation(self, layer, key):
        """the saved activation ``key`` ("r", "xn0", "xn1", ...) of encoder layer ``layer`` of the LAST step (tests, diagnostics)"""
        return self.layers[layer][key]

    def _refresh_transposes(self):
        if self.n_out > 1:                                        # W_out^T [d, d_output] zero-padded to a multiple of 4 columns
            self.woutT_pad[:, :self.n_out].copy_(self.head.w.t())
        if self.gemm == "hipblaslt":
            return
        w0 = self.fc[0].w if self._x_pad else None
        if self._fused_images:
            pad = (w0, self.w0_pad, self.w0_pad_i) if self._x_pad else ()
            KN.weight_images(self.lib, self._st(), self.flat_p, self.flat_pi, self.flat_t, self.flat_ti, self._tdesc, self._tstart, self._tn,
                             self._ttiles if self._tn else 0, *pad)
            return
        if self._x_pad:
            self.w0_pad[:, :w0.shape[1]].copy_(w0)
            KN.split_image(self.lib, self._st(), self.w0_pad, self.w0_pad_i, "split_image(W0 padded)")
        if self._tn:
            KN.transpose_batch(self.lib, self._st(), self.flat_p, self.flat_t, self._tdesc, self._tstart, self._tn, self._ttiles)
            KN.split_image(self.lib, self._st(), self.flat_t, self.flat_ti, "split_image(W^T)")
        KN.split_image(self.lib, self._st(), self.flat_p, self.flat_pi, "split_image(W)")

    def _sync_weights(self):
        """The forward / input-gradient GEMMs read the pre-split images and transposed copies of the weights, which the step
        refreshes after its own optimizer update.  A weight change made from OUTSIDE (``model.load_state_dict(ckpt)``, a manual
        re-initialisation, an external optimizer on the aliased parameters) bumps the parameters' autograd version counters --
        kernel writes through raw pointers do not -- so a changed counter (or a step of the slate-resident FC path, which never
        touches the images) means: refresh before the next forward."""
        ver = [r.p._version for r in self.params]
        if ver != self._wver or self._images_stale:
            self._refresh_transposes()
            self._wver = [r.p._version for r in self.params]
            self._images_stale = False

    def _bucket_done(self, k):
        """gradient bucket k is final: start its all-reduce(SUM) now, behind the rest of the backward (the collective runs
        on the process group's own stream; ``_full`` waits for all of them before the optimizer step).  While a step is being
        captured the collective is not issued but handed to ``_seg_break``: it ends the hipGraph segment recorded so far and
        is launched between that segment's replay and the next one's."""
        if self.sharded and self.comm_enabled:
            import torch.distributed as dist
            lo, hi = self._buckets[k]
            if hi > lo:
                def launch(lo=lo, hi=hi):
                    self._works.append(dist.all_reduce(self.flat_g[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
                if self._seg_break is not None:
                    self._seg_break(launch)
                else:
                    launch()

    def _wait_buckets(self):
        def wait():
            for w_ in self._works:                               # bucketed gradient all-reduces launched during the backward
                w_.wait()
            self._works = []
        if self._seg_break is not None and self.sharded and self.comm_enabled:
            self._seg_break(wait)
        else:
            wait()

    def _relu_bits(self, st):
        """the one-bit ReLU mask buffer of a layer's feed-forward activation for THIS step's row count, or None where the form does
        not apply (ltrx_gemm_nt_relu_bits_bytes: the large-tile GEMM must run both launches) -- then the input-gradient GEMM reads
        the saved fp32 activation instead (act 2)"""
        buf = st.get("rbits")
        if buf is None or self.gemm in ("hipblaslt", "split_bf16_strict"):
            return None
        # (both launches of a mask -- FFN-1 forward and FFN-2 input gradient -- contract over d_model: one K to ask about)
        need = self.lib.ltrx_gemm_nt_relu_bits_bytes(self.rows, self.dff, self.d)
        return buf if 0 < need <= buf.numel() else None

    def _gemm_nt(self, a, b, b_img, out, M, bias, act, aux, p, seed, what):
        """the ltrx_gemm_nt launch of the step: out[:M] = epi_act(a b^T + bias), dropout (p, site ``seed``) in the epilogue; ``aux`` as
        the act code reads it (include/ltrx.h); ``b_img``: the address of ``b``'s split image, or None"""
        KN.gemm_nt(self.lib, self._st(), a, b, out, M, bias, act, aux, p, seed, self.drop_step, self._prec, 0, b_img, what)

    def _lin_fwd(self, x, lin, out, act=0, p=0.0, seed=0, res=None, bits=None, rows=None):
        """out = drop_p(act(x w^T + b)) [+ res]   (the forward of the projection ``lin``, act 1 = ReLU; dropout in the epilogue; ``res`` = the
        residual stream of the SublayerConnection this projection closes, transformer.py:98-106: added in the epilogue, so the
        sum is written once by the GEMM instead of being re-read and re-written by the LayerNorm that follows; ``rows``: the row
        count of the pass, default the step's)"""
        M = self.rows if rows is None else rows
        b = lin.b
        if self.gemm == "hipblaslt":
            n = M
            torch.addmm(b, x[:n], lin.w.t(), out=out[:n])
            if act == 1:
                torch.relu_(out[:n])
            if p:
                self._drop_apply(out, out, p, seed)
            if res is not None:
                out[:n].add_(res[:n])
            return
        # (the first FC layer over padded input rows multiplies the zero-padded copy of its weight)
        w, img = (lin.w, lin.w_img) if lin.w_pad is None else (lin.w_pad, lin.w_pad_img)
        if bits is not None and act == 1:                         # ReLU + its one-bit mask for the backward (act 4)
            self._gemm_nt(x, w, img, out, M, b, 4, bits, p, seed, "gemm_nt(fwd, relu bits)")
        elif res is not None:
            self._gemm_nt(x, w, img, out, M, b, 3, res, p, seed, "gemm_nt(fwd)")
        else:
            self._gemm_nt(x, w, img, out, M, b, act, None, p, seed, "gemm_nt(fwd)")

    def _lin_dgrad(self, dy, lin, out, relu_of=None, p=0.0, seed=0, bits=None):
        """out = dy w   (input gradient of the projection ``lin``, through its contiguous w^T).  With ``relu_of`` (the saved post-ReLU,
        post-dropout activation that produced the layer input) the ReLU(+dropout p) backward mask is applied in the GEMM
        epilogue; without it, p > 0 re-applies the dropout mask of site ``seed`` (identity activation)."""
        if self.gemm == "hipblaslt":
            torch.mm(dy[:self.rows, :lin.w.shape[0]], lin.w, out=out[:self.rows])      # (dy may carry zero padding columns)
            if relu_of is not None:
                self._relu_bwd(out, relu_of, p)
            elif p:
                self._drop_apply(out, out, p, seed)
            return
        wT, img = lin.wT, lin.wT_img
        if relu_of is None:
            self._gemm_nt(dy, wT, img, out, self.rows, None, 0, None, p, seed, "gemm_nt(dgrad)")
        elif bits is not None:                                    # the mask written by the forward launch (act 5): 1/32 of the bytes
            self._gemm_nt(dy, wT, img, out, self.rows, None, 5, bits, p, seed, "gemm_nt(dgrad, relu bits)")
        else:
            self._gemm_nt(dy, wT, img, out, self.rows, None, 2, relu_of, p, seed, "gemm_nt(dgrad)")

    def _lin_wgrad(self, dy, x, lin, defer=False):
        """lin.gw = dy^T x, lin.gb = column sums of dy   (weight and bias gradients of the projection).  ``defer``: an encoder-layer projection
        -- queued for the layer's one grouped launch (_wgrad_flush); dy and x must stay untouched until then."""
        gw, gb = lin.gw, lin.gb
        if self.gemm == "hipblaslt":
            torch.mm(dy[:self.rows].t(), x[:self.rows], out=gw)
            self._colsum(dy, gb)
            return
        if defer and self.group_wgrad:
            self._wg_pending.append((dy, x, gw, gb))
            return
        # (tile 9: x is the padded input buffer -- its rows are readable up to the 256-column tile, see include/ltrx.h)
        padded = self._x_large and x.data_ptr() == self.x_in_buf.data_ptr() and x.stride(0) == self.x_in_buf.stride(0)
        KN.gemm_tn(self.lib, self._st(), dy, x, gw, gb, self.rows, self._prec, 9 if padded else 0, self.ws_tn, "gemm_tn(wgrad)")

    def _wgrad_flush(self, defer_reduce=False, ln=None):
        """the queued weight gradients of a layer as ONE ltrx_gemm_tn_group launch; their partial slabs are summed by the call
        (one launch per projection) or, with ``defer_reduce``, by the layer's _reduce_flush (the workspace must stay untouched
        until then).  ``ln``: the arguments of a _ln_bwd call that is due right after the launch and writes none of its operands --
        the call then covers both (ltrx_gemm_tn_group_ln: the LayerNorm backward in the launch's idle CUs where the library takes it)."""
        q = self._wg_pending
        buf = self._ln_partial_slot() if (ln is not None and q) else None
        if ln is not None and buf is None:                        # nothing queued, or no deferred reduction: the plain pair
            self._wgrad_flush(defer_reduce)
            self._ln_bwd(*ln)
            return
        if not q:
            return
        n = len(q)
        # did the grouped kernel take this composition, or did the call fall back to one launch per problem (shapes outside the
        # large-tile kernel / not enough workspace)?  The host-side predicate the library applies, asked of the library with the
        # arguments of the call below; tests assert it
        took = KN.tn_group_plan(self.lib, q, self.rows, self._prec, self.ws_tn)
        self.wgrad_group_log.append((n, took))
        del self.wgrad_group_log[:-16]
        if self.probe_wgrad is not None:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        if ln is None:
            slabs = KN.gemm_tn_group(self.lib, self._st(), q, self.rows, self._prec, self.ws_tn, defer_reduce, "gemm_tn_group(wgrad)")
        else:
            dy, xsum, nm, mean, rstd, dres, dx = ln
            slabs, ln_rows, side = KN.gemm_tn_group_ln(self.lib, self._st(), q, self.rows, self._prec, self.ws_tn, dy, xsum, nm.a, mean, rstd,
                                                       dres, nm.eps, dx, buf, defer_reduce,
                                                       "gemm_tn_group_ln(wgrad + layernorm_bwd)")
            self.ln_side_log.append(side)
            del self.ln_side_log[:-16]
        if self.probe_wgrad is not None:
            ev1.record()
            self.probe_wgrad.append((ev0, ev1, n, took))
        if defer_reduce and slabs[2] > 0:
            so, bso, splits = slabs
            for i, t in enumerate(q):
                nw = t[0].shape[1] * t[1].shape[1]
                self._red_pending.append((so[i], splits, nw, nw, t[2].data_ptr()))
                if bso[i]:
                    self._red_pending.append((bso[i], splits, t[0].shape[1], t[0].shape[1], t[3].data_ptr()))
        if ln is not None:                                        # (after the slabs: the queue position _ln_bwd's entries had)
            self._ln_partials_queue(buf, ln_rows, nm.ga, nm.gb)
        q.clear()

    def _reduce_flush(self):
        """every pending fixed-order reduction of the layer (weight-gradient slabs, bias column sums, LayerNorm parameter-gradient
        partials) in ONE launch (ltrx_reduce_group)"""
        q = self._red_pending
        self._ln_slot = 0
        if not q:
            return
        KN.reduce_group(self.lib, self._st(), q)
        q.clear()

    # ---- the step body (capturable) ----------------------------------------------------------------------------
    def _forward(self, train=True, bs=None):
        """input buffers -> scores of the buffer set ``bs`` (what that is: ``_alloc_forward``): the step's own (``bs`` None = self) or
        a FusedScorer's (the valid-row count is then read from its device cu_seqlens).  ``train=False`` is model.eval(): every dropout
        rate is 0 (the activations are written all the same).  Returns (feat, sc_rows)."""
        bs = self if bs is None else bs
        lib, M, d, B, L = self.lib, bs.rows, self.d, bs.B, bs.L
        stream = self._st()                                       # (of the row movers: the pass stays on one stream)
        kpm = bs.mask if bs.layout == "grid" else None            # packed rows are all valid keys
        dp = (lambda p: p) if train else (lambda p: 0.0)          # dropout rate of a site in this pass
        h = bs.x_in
        nm = self.norm_in
        if nm is not None and self._x_pad:                        # ... into the first F columns of the padded operand rows
            KN.layernorm_torch_fwd_strided(lib, self._st(), h, nm.a, nm.b, M, nm.eps, bs.x_norm, bs.mean_in, bs.rstd_in)
            h = bs.x_norm
        elif nm is not None:                                      # FCModel.input_norm (model.py:39)
            KN.layernorm_torch_fwd(lib, self._st(), h, nm.a, nm.b, M, nm.eps, bs.x_norm, bs.mean_in, bs.rstd_in)
            h = bs.x_norm
        for i, lin in enumerate(self.fc):
            if lin.w_pad is not None:                              # F rounded up to the GEMM's K step: padded rows x padded W_0
                h = bs.x_in_k                                      # (hipblaslt has no w_pad: torch.addmm over the [:, :F] view and W_0 itself)
            if self.fc_act >= 3:                                   # Sigmoid / Tanh: GEMM + bias, then the activation in place
                self._lin_fwd(h, lin, bs.fc_out[i], rows=M)
                KN.out_act_fwd(lib, self._st(), bs.fc_out[i], M * bs.fc_out[i].shape[1], self.fc_act - 2, bs.fc_out[i], "fc_act_fwd")
            else:
                self._lin_fwd(h, lin, bs.fc_out[i], self.fc_act, dp(self.p_fc), self._site(1000 + i), rows=M)
            h = bs.fc_out[i]
        if self.pos is not None:                                  # transformer.py:51-52: x = sqrt(d) x + pe[rank]
            KN.posenc_fwd(lib, self._st(), h, self.pos_table, bs.idx_rows, kpm, M, self.pos_pad, float(d) ** 0.5, bs.x_pe)
            h = bs.x_pe
        x = h                                                     # residual stream
        for i, st in enumerate(bs.layers):
            self._ln_fwd(x, None, st["norm0"], None, st["xn0"], st["mean0"], st["rstd0"], rows=M)
            st["xin"] = x
            self._lin_fwd(st["xn0"], st["lin_qkv"], st["qkv"], rows=M)
            KN.mha_fwd(lib, self._st(), st["q"], st["k"], st["v"], kpm, B, L, self.h, st["o"], st["lse"], dp(st["p_att"]), st["s_att"],
                       self.drop_step, bs.cu, bs.order, self._mha_mode)
            RW.zero_attention_tail(bs, lib, stream, st["o"])
            # x1 = x + dropout(attention branch): the residual sum is the out-projection's epilogue (act 3)
            self._lin_fwd(st["o"], st["lin_o"], st["x1"], 0, dp(st["p_s0"]), st["s_s0"], res=x, rows=M)
            self._ln_fwd(st["x1"], None, st["norm1"], None, st["xn1"], st["mean1"], st["rstd1"], rows=M)
            if self.probe is not None and train:                  # bench.py: HIP events around the roofline kernel, in the step
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
            self._lin_fwd(st["xn1"], st["lin_ff1"], st["r"], 1, dp(st["p_ff"]), st["s_ff"],
                          bits=self._relu_bits(st) if train else None, rows=M)
            if self.probe is not None and train:
                ev1.record()
                self.probe.append((ev0, ev1))
            # x(next layer) = x1 + dropout(feed-forward branch), again in the epilogue of the projection that closes the sublayer
            nxt = bs.layers[i + 1]["xsum0"] if i + 1 < len(bs.layers) else bs.xsum_f
            self._lin_fwd(st["r"], st["lin_ff2"], nxt, 0, dp(st["p_s1"]), st["s_s1"], res=st["x1"], rows=M)
            x = nxt
        nf, head, no = self.norm_f, self.head, self.n_out
        sc_rows = bs.scores_raw if bs.layout == "grid" else bs.scores_c
        feat = x
        if self.N and not self.norm_head:
            self._ln_fwd(x, None, nf, None, bs.xf, bs.mean_f, bs.rstd_f, rows=M)
            feat = bs.xf
        if self.norm_head:                                        # final norm + score head in one pass: LN(x) stays in registers
            feat = None
            KN.norm_head_fwd(lib, self._st(), x, nf.a, nf.b, head.w, head.b, M, nf.eps, sc_rows, bs.mean_f, bs.rstd_f)
        elif no == 1:
            KN.score_head_fwd(lib, self._st(), feat, head.w, head.b, M, sc_rows)
        else:                                                     # Linear(d, d_output) as a GEMM (model.py:117)
            self._lin_fwd(feat, head, sc_rows.view(-1, no), rows=M)
        if self.out_act:                                          # OutputLayer activation (model.py:117), in place
            KN.out_act_fwd(lib, self._st(), sc_rows, M * no, self.out_act, sc_rows)
        RW.scores_to_grid(bs, lib, stream, sc_rows, no)           # packed scores -> the padded [B, L] grid of the loss kernels
        if no > 1:
            torch.sum(bs.scores_raw, dim=-1, out=bs.scores)       # model.score (model.py:127)
        return feat, sc_rows

    def _body(self):
        lib, M, d, B, L = self.lib, self.rows, self.d, self.B, self.L
        stream = self._st()                                       # (of the row movers)
        kpm = self.mask if self.layout == "grid" else None
        nf, head, no = self.norm_f, self.head, self.n_out
        self._wg_pending.clear()                                  # (a step that raised half-way must not leave work queued)
        self._red_pending.clear()
        self._ln_slot = 0
        feat, sc_rows = self._forward(True)
        # ---------------- loss (value + d/dscores) ----------------
        loss, dsc = self.loss.run(self.scores_raw, self.y_in, self._divisor)
        # ---------------- backward ----------------
        ga, gb = self.d_a, self.d_b
        spare = self.d_c if (self.N and self.ln_in_wgrad) else None
        dsc = RW.grid_to_rows(self, lib, stream, dsc, no)         # d loss / d scores of the packed rows (alignment rows: 0)
        if self.out_act:                                          # d loss / d pre-activation = d loss / d score * act'(score)
            KN.out_act_bwd(lib, self._st(), dsc, sc_rows, M * no, self.out_act, dsc)
        if self.norm_head:
            # backward of the fused pair.  The head's own gradients first, in ltrx_score_head_bwd's row order (their bits), from the
            # recomputed LN(x); then d_xf = dsc w is formed in registers and dx lands where _ln_bwd put it, the (a_2, b_2) partials
            # joining the last layer's one reducing launch as _ln_bwd's do
            KN.norm_head_wgrad(lib, self._st(), dsc, self.xsum_f, nf.a, nf.b, self.mean_f, self.rstd_f, M, head.gw, head.gb, self.ws_head)
            buf = self._ln_partial_slot()                         # (never None: norm_head implies the deferred reduction, slot 0)
            nrows = KN.norm_head_bwd_partial(lib, self._st(), dsc, self.xsum_f, nf.a, head.w, self.mean_f, self.rstd_f, M, nf.eps, gb, buf)
            self._ln_partials_queue(buf, nrows, nf.ga, nf.gb)
        elif no == 1:
            KN.score_head_bwd(lib, self._st(), dsc, feat, head.w, M, ga, head.gw, head.gb, self.ws_head)
        else:                                                     # the d_output-wide head: weight / bias / input gradients as GEMMs
            self.dz_pad[:M, :no].copy_(dsc.reshape(-1, no)[:M])
            self._lin_wgrad(self.dz_pad[:, :no], feat, head)
            self._lin_dgrad(self.dz_pad, head, ga)                # (through woutT_pad)
        if self.N:
            if not self.norm_head:
                self._ln_bwd(ga, self.xsum_f, nf, self.mean_f, self.rstd_f, None, gb)
            ds = gb                                               # d loss / d (x1_last + ffn_last)
            other = ga
            for i in range(self.N - 1, -1, -1):
                st = self.layers[i]
                d_r, dqkv = self.d_r, self.dqkv
                # where the two LayerNorm backwards of the layer write: ping-pong over (ga, gb); with ln_in_wgrad the second one runs
                # WHILE the weight gradients read ds (the FFN-2 dY operand), so it writes a third buffer and the three rotate
                mid, outb, d_top = other, (ds if spare is None else spare), ds
                # FFN branch
                db = self._branch_grad(ds, st["p_s1"], st["s_s1"])
                # (the four weight gradients of the layer are queued and run as one grouped launch before the first kernel that
                #  overwrites one of their operands: the LN0 backward below, or the second use of the dropout buffer d_br)
                self._lin_wgrad(db, st["r"], st["lin_ff2"], defer=True)
                self._lin_dgrad(db, st["lin_ff2"], d_r, relu_of=st["r"], p=st["p_ff"], bits=self._relu_bits(st))
                self._lin_wgrad(d_r, st["xn1"], st["lin_ff1"], defer=True)
                self._lin_dgrad(d_r, st["lin_ff1"], self.tmp_d)
                self._ln_bwd(self.tmp_d, st["x1"], st["norm1"], st["mean1"], st["rstd1"], ds, mid)
                ds = mid                                           # ds = d loss / d x1
                # attention branch
                if st["p_s0"] and st["p_s1"]:                      # d_br still holds the FFN branch's dY
                    self._wgrad_flush()
                db = self._branch_grad(ds, st["p_s0"], st["s_s0"])
                self._lin_wgrad(db, st["o"], st["lin_o"], defer=True)
                self._lin_dgrad(db, st["lin_o"], self.d_o)
                KN.mha_bwd(lib, self._st(), st["q"], st["k"], st["v"], kpm, st["o"], self.d_o, st["lse"], B, L, self.h, self.dq, self.dk,
                           self.dv, st["p_att"], st["s_att"], self.drop_step, self.cu, self.order, self._mha_mode, self.ws_mha)
                RW.zero_gradient_tail(self, lib, stream, dqkv)
                self._lin_wgrad(dqkv, st["xn0"], st["lin_qkv"], defer=True)
                self._lin_dgrad(dqkv, st["lin_qkv"], self.tmp_d)
                ln0 = (self.tmp_d, st["xin"], st["norm0"], st["mean0"], st["rstd0"], ds, outb)
                if spare is None:
                    self._wgrad_flush(defer_reduce=True)
                    self._ln_bwd(*ln0)
                    ds, other = outb, mid                          # ds = d loss / d (layer input)
                else:
                    self._wgrad_flush(defer_reduce=True, ln=ln0)
                    ds, other, spare = outb, mid, d_top            # (the layer's incoming gradient is free in the next layer)
                self._reduce_flush()                               # the layer's parameter gradients are final from here
                self._bucket_done(self.N - 1 - i)
        else:
            ds, other = ga, gb
        if self.pos is not None:                                  # backward of x = sqrt(d) fc_out + pe[rank]
            if self.pos_learned:
                KN.posenc_table_bwd(lib, self._st(), ds, self.idx_rows, kpm, M, self.pos_pad, self.pos_g)
            KN.scale_inplace(lib, self._st(), ds, M * d, float(d) ** 0.5)
        # FC stack
        for i in range(self.nfc - 1, -1, -1):
            lin = self.fc[i]
            if i == self.nfc - 1:                                # the last FC activation(+dropout) feeds the encoder / head
                if self.fc_act >= 3:
                    KN.out_act_bwd(lib, self._st(), ds, self.fc_out[i], M * ds.shape[1], self.fc_act - 2, ds, "fc_act_bwd")
                elif self.fc_act == 1:
                    self._relu_bwd(ds, self.fc_out[i], self.p_fc)
                elif self.p_fc:
                    self._drop_apply(ds, ds, self.p_fc, self._site(1000 + i))
            inp = (self.x_norm if self.in_norm is not None else self.x_in) if i == 0 else self.fc_out[i - 1]
            self._lin_wgrad(ds, inp, lin)
            if i == 0 and self.in_norm is not None:
                # nn.LayerNorm parameter gradients: dw = sum dy * xhat, db = sum dy with dy = ds W_0 (the input itself needs no
                # gradient; ltrx_layernorm_bwd's da / db formulas only use the saved mean and rstd, its dx output is scratch)
                nm = self.norm_in
                self._lin_dgrad(ds, lin, self.d_in)
                KN.layernorm_bwd(lib, self._st(), self.d_in, self.x_in, nm.a, self.mean_in, self.rstd_in, None, M, nm.eps, self.d_in, nm.ga,
                                 nm.gb, self.ws_ln_in, "layernorm_bwd(input_norm)")
            if i > 0:
                self._lin_dgrad(ds, lin, self.fc_dgrad[i - 1],
                                relu_of=self.fc_out[i - 1] if self.fc_act == 1 else None, p=self.p_fc,
                                seed=self._site(1000 + i - 1))
                ds = self.fc_dgrad[i - 1]
                if self.fc_act >= 3:
                    KN.out_act_bwd(lib, self._st(), ds, self.fc_out[i - 1], M * ds.shape[1], self.fc_act - 2, ds, "fc_act_bwd")
        self._bucket_done(len(self._buckets) - 1)
        return loss

    def _adam(self):
        if self.clip:
            KN.clip_grad_norm_scale(self.lib, self._st(), self.flat_g, self.clip, self.clip_scale, self.grad_norm, self.ws_clip)
        gsc = self.clip_scale if self.clip else None
        if self.optimizer == "SGD":
            KN.sgd_step(self.lib, self._st(), self.flat_p, self.flat_g, self.flat_m if self.momentum else None, self.lr, self.momentum,
                        self.nesterov, self.weight_decay, gsc)
            return
        KN.adam_step(self.lib, self._st(), self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.lr, self.betas, self.eps,
                     self.weight_decay, self.optimizer == "AdamW", self.step_count, gsc)

    def _full(self):
        if self._any_dropout or self.loss.stochastic:
            KN.bump_u32(self.lib, self._st(), self.drop_step)    # fresh masks / noise every step
        loss = self._body()
        self._wait_buckets()
        self._adam()
        self._refresh_transposes()
        return loss

    def first_nonfinite(self):
        """(name of the first parameter tensor -- flat-buffer order -- whose gradient of the LAST step holds a NaN / Inf, number of
        non-finite gradient elements), or (None, 0): the finiteness check that stands in for torch.autograd.detect_anomaly() on a
        step without an autograd graph (main.py:89).  One launch over the flat gradient buffer, one host sync."""
        if getattr(self, "_nf_seg", None) is None:
            self._nf_names = [r.name for r in self.params]
            self._nf_seg = torch.tensor([r.off for r in self.params], dtype=torch.int64, device=self.dev)
            self._nf_out = torch.zeros(2, dtype=torch.int32, device=self.dev)
        KN.first_nonfinite(self.lib, self._st(), self.flat_g, self._nf_seg, self._nf_out)
        first, count = (int(v) for v in self._nf_out.cpu())
        return (self._nf_names[first], count) if count else (None, 0)

    def set_lr(self, lr):
        """change the learning rate (per-epoch scheduler step): the rate is a launch argument of the Adam kernel, so a
        captured graph is dropped and re-captured on the next step (the warm-up counts stay: no new eager steps)"""
        if float(lr) != float(self.lr):
            self.lr = float(lr)
            self._graphs.clear()

    # ---- checkpointing: the state of a fused run that neither the nn.Module nor the torch.optim object sees ------------------------
    def _moment_slots(self):
        """the optimizer's moment slots in the neutral schema of allrank_amd.checkpoint, each with the flat buffer that holds it
        (1: flat_m, 2: flat_v)"""
        return (("momentum_buffer", 1),) if self.optimizer == "SGD" else (("exp_avg", 1), ("exp_avg_sq", 2))

    def _hyper(self):
        from . import checkpoint as CK
        return CK.hyper(self.optimizer, self.lr, self.betas, self.eps, self.weight_decay, self.momentum, self.nesterov)

    def meta(self):
        """what ``checkpoint.check_compatible`` compares: parameter names / shapes, optimizer kind and hyper-parameters, loss, clipping"""
        from . import checkpoint as CK
        return CK.make_meta([(r.name, r.p) for r in self._params_named], self.optimizer, self._hyper(), self.loss.name, self._loss_args,
                            self.clip)

    def state_dict(self):
        """Everything a resumed run needs to be THIS run, as CPU tensors and plain values (one device-to-host copy, one host sync):
        ``params`` by parameter name, the optimizer moments in the neutral schema of allrank_amd.checkpoint (unpadded, shaped like
        the parameters: neither the 4-float segment padding nor the q / k / v adjacency of the flat buffers reaches the file) with
        ``step`` from the device step count, the dropout / noise step word ``drop_step`` (as u32), the generator ``seed``, ``lr``,
        the state of the ListMLE tie-shuffle generator, and the ``meta`` block.  Not state: B, L, the row layout, the gemm mode,
        graphs and workspaces, scorers."""
        n = self.nflat
        host = torch.cat([self.flat_p, self.flat_m, self.flat_v, self.step_count, self.drop_step.view(torch.float32)]).cpu()
        step, word = int(host[3 * n].item()), int(host[3 * n + 1:].view(torch.int32).item()) & 0xFFFFFFFF
        params, moments = {}, {}
        for r in self._params_named:
            seg = lambda k: host[k * n + r.off:k * n + r.off + r.w.numel()].view(r.w.shape).clone()
            params[r.name] = seg(0)
            moments[r.name] = {slot: seg(k) for slot, k in self._moment_slots()}
        return {"params": params,
                "optimizer": {"kind": self.optimizer, "hyper": self._hyper(), "step": step, "state": moments},
                "drop_step": word, "seed": int(self._seed), "lr": float(self.lr), "perm_gen": self._perm_gen.get_state().cpu().clone(),
                "meta": self.meta()}

    def load_state_dict(self, sd):
        """Put a ``state_dict()`` (of this engine, or the autograd engine's neutral one) back IN PLACE: ``copy_`` into the flat
        buffers, ``fill_`` on the two device words -- no buffer is rebound, so captured graphs, the module's parameters and the raw
        pointers of the slate-resident step stay valid; the segments' padding floats stay zero.  The weight images, transposes and
        padded copies are marked stale (the next forward refreshes them: nothing bumps an autograd version counter here), the
        learning rate goes through ``set_lr``, and another seed re-keys every dropout site and the stochastic loss and drops the
        captured steps and ``score()``'s capture (site seeds are by-value launch arguments).  Compatibility is checked first: a
        refusal (ValueError) leaves the trainer untouched."""
        from . import checkpoint as CK
        CK.check_compatible(sd["meta"], self.meta())
        opt = sd["optimizer"]
        if "state" not in opt:
            raise ValueError("checkpoint: the stored optimizer state is a raw torch %s state_dict: only the autograd engine resumes it"
                             % (opt.get("kind"),))
        n = self.nflat
        host = torch.zeros(3 * n, dtype=torch.float32)
        for r in self._params_named:
            name, o, shape = r.name, r.off, r.w.shape
            srcs = [(sd["params"].get(name), 0)] + [(opt["state"].get(name, {}).get(slot), k) for slot, k in self._moment_slots()]
            for t, k in srcs:
                if t is None or tuple(t.shape) != tuple(shape):
                    raise ValueError("checkpoint: parameter %s: no tensor of shape %s in the %s" % (name, tuple(shape), "parameters" if k == 0 else "optimizer state"))
                host[k * n + o:k * n + o + r.w.numel()].copy_(t.reshape(-1))
        dev = host.to(self.dev)
        self.flat_p.copy_(dev[:n])
        self.flat_m.copy_(dev[n:2 * n])
        self.flat_v.copy_(dev[2 * n:])
        self.step_count.fill_(float(int(opt["step"])))
        if sd.get("drop_step") is not None:
            word = int(sd["drop_step"]) & 0xFFFFFFFF
            self.drop_step.fill_(word - (1 << 32) if word >= (1 << 31) else word)
        self._images_stale = True
        self.set_lr(float(sd["lr"]))
        if sd.get("seed") is not None and int(sd["seed"]) != self._seed:
            self._seed = int(sd["seed"]) & 0xFFFFFFFF
            sites, noise = self._site_seeds()
            for ops, st, seeds in zip(self._layer_ops, self.layers, sites):
                ops.update(seeds)
                st.update(seeds)
            self._graphs.clear()
            self._fwd_graphs.graphs.clear()
            if self.loss.stochastic:
                self.loss.set_noise_key(noise, self.drop_step)
        if sd.get("perm_gen") is not None:
            self._perm_gen.set_state(sd["perm_gen"].to(torch.uint8).cpu())

    def _pack(self, xb, lengths):
        """compact mode: build idx / cu_seqlens for this batch and gather the valid rows of xb into x_in.  ``lengths`` (host
        ints, one per slate; valid items first, as dataset.py:28-38 pads) avoids the one host sync that counting the
        valid items on the device costs."""
        B, L = self.B, self.L
        if lengths is not None:
            # only the B+1 prefix sums and the launch order cross PCIe (_Stager); the packed-row index is derived on the device
            n = self._stager.upload(torch.as_tensor(lengths, dtype=torch.int32).reshape(B).clamp(min=0, max=L))
            KN.packed_row_index(self.lib, self._st(), self.cu, B, L, n, self.idx)
        else:
            valid = (self.mask == 0)
            cnt = valid.sum(1)
            self.cu[1:] = torch.cumsum(cnt, 0)
            self.order.copy_(torch.argsort(cnt, descending=True, stable=True))
            idx = torch.nonzero(valid.reshape(-1)).reshape(-1)    # (host sync: the row count sizes every launch)
            n = int(idx.numel())
            self.idx[:n] = idx
        if n == 0 and not self.sharded:
            raise ValueError("FusedTrainer(compact=True): the batch has no valid item")
        # (sharded: a rank whose block of a short last batch is empty -- 1 slate on 2 ranks -- still runs the step on 32 all-zero
        #  alignment rows: zero loss, zero gradient, and every collective of the step is entered by every rank)
        self.n_valid = n
        # alignment rows (zero input, zero gradient) keep the row count a multiple of 32; never more rows than the buffers hold
        # (a tiny batch, B * L < 32: the old max(32, ...) ran 32 rows over M-row buffers -- ADVICE r4)
        self.rows = min(self.M, max(32, (n + 31) // 32 * 32))
        KN.gather_rows(self.lib, self._st(), xb, self.idx, n, self.rows, self.x_in.shape[1], self.x_in)

    def bucket_of(self, counts):
        """compact="graph": the rows a step over batches of ``counts`` valid items runs -- ``row_bucket``, the scorer's ladder,
        capped at the rows the buffers hold"""
        return [row_bucket(max(int(n), 1), self.cap) for n in counts]

    def _pack_cu(self, xb, indices, lengths):
        """compact="graph" staging (``rows.stage_cu``, outside any capture).  Host ``lengths``: no sync.  Without them the slates are
        counted on the device -- one sync, which also checks that the valid items of every slate come first (what the cu_seqlens
        kernels assume)."""
        def check(got):
            if not got.get("prefix_ok", 1):
                raise ValueError("FusedTrainer(compact=\"graph\"): a slate has padding between its valid items -- the captured step packs "
                                 "from cu_seqlens, which needs the valid items first in every slate (compact=True takes such a batch)")
            if got["n"] == 0:
                raise ValueError("FusedTrainer(compact=\"graph\"): the batch has no valid item")
        if lengths is not None:
            lengths = torch.as_tensor(lengths, dtype=torch.int32).reshape(self.B).clamp(min=0, max=self.L)
        RW.stage_cu(self, self.lib, self._st(), xb, indices if self.pos is not None else None, lengths,
                    valid=None if lengths is not None else self.mask == 0, want=("n", "prefix_ok"), check=check)

    def _reattach(self):
        """the module's parameters / gradients must alias the flat buffers (state_dict(), score() and external readers of
        .grad see what the kernels wrote): re-point anything an external zero_grad(set_to_none=True) / .to() detached."""
        for _, p, _, w, g in self.params:
            if p.data.data_ptr() != w.data_ptr():
                p.data = w
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g

    def _stage_batch(self, xb, yb, indices, lengths, who):
        """the batch of ``step()`` / ``score()`` into the static input buffers: labels, padding mask and features (one launch where
        the caller's tensors allow it), the packed rows when compact, the rank of every row when the model has a positional encoding"""
        self.y_cur = self.y_in
        direct = (yb.dtype == torch.float32 and yb.is_contiguous() and yb.is_cuda and yb.numel() == self.M
                  and (self.compact or (xb.dtype == torch.float32 and xb.is_contiguous() and xb.is_cuda
                                        and xb.numel() == self.x_in.numel())))
        if direct:                                                # x, y and the padding mask in one launch
            KN.ingest_batch(self.lib, self._st(), None if self.compact else xb, yb, PADDED_Y_VALUE, self.x_in, self.y_in, self.mask)
        else:
            self.y_in.copy_(yb)
            self.mask.copy_(yb == PADDED_Y_VALUE)
        if self.pos is not None and indices is None:
            raise ValueError("FusedTrainer: the model has a positional encoding, %s() needs `indices`" % who)
        if self.layout == "cu":                                   # (the positions move with the features)
            self._pack_cu(xb.to(self.dev, torch.float32).reshape(self.M, -1).contiguous(), indices, lengths)
        elif self.layout == "index":
            self._pack(xb.reshape(self.M, -1).contiguous(), lengths)
            if self.pos is not None:                              # rank of every packed row; alignment rows -> padding row
                self.idx_rows.fill_(-1)
                self.idx_rows[:self.n_valid] = indices.reshape(-1)[self.idx[:self.n_valid].long()]
        else:
            if not direct:
                self.x_in.copy_(xb.reshape(self.M, -1))
            if self.pos is not None:
                self.idx_rows.copy_(indices.reshape(-1))

    scanned = "gradient"                          # what first_nonfinite() reads

    def _block(self, xb, yb, indices, lengths):
        """a block of up to B slates topped up to the static shape: fully padded slates and, where packed rows run, zero lengths"""
        n = int(xb.shape[0])
        if not self.compact:
            lengths = None
        elif lengths is not None and n < self.B:
            lengths = torch.cat([lengths, lengths.new_zeros(self.B - n)])
        return pad_batch(xb, yb, indices, self.B) + (lengths,)

    def step_block(self, xb, yb, indices, global_batch, lengths=None):
        """``step`` on this rank's block of a global batch of ``global_batch`` slates as the loader delivered it, short or empty (the
        loss is normalised by the real slate count); returns the loss and leaves ``scores[:n]`` / ``y_cur[:n]`` of the step"""
        xs, ys, ids, lengths = self._block(xb, yb, indices, lengths)
        return self.step(xs, ys, ids, global_batch=global_batch, lengths=lengths)

    def step(self, xb, yb, indices=None, global_batch=None, lengths=None):
        """copy the batch into the static input buffers and run (or replay) the step; returns the device loss [1]."""
        self._reattach()
        if self.fcstep:
            return self._fc_step(xb, yb, global_batch)
        self._sync_weights()
        if self.loss.name == "listMLE" and self.shuffle_ties:
            # listMLE.py:17: a fresh random column order per call breaks ties among equal labels at random; the
            # permutation lives in a persistent device buffer, so the refresh is safe under hipGraph replay
            self.loss.perm.copy_(torch.randperm(self.L, device=self.dev, generator=self._perm_gen))
        key = self._key(global_batch)
        self._divisor = key[0]
        self._stage_batch(xb, yb, indices, lengths, "step")
        if self.layout == "cu":                                   # the staging picked the row bucket: the third part of the key
            key = self._key(global_batch)
            self.bucket_counts[self.rows] += 1
        if self.use_graph:
            live = key in self._graphs
            self._captured(key)                                   # (a failed capture of a sharded step turns use_graph off for good)
        if self.use_graph:
            mode = self._step_graphs.run(key, self._eager)        # warm-up step, or replay
            self.last_mode = "capture" if (mode == "replay" and not live) else mode      # (recorded just above, replayed here)
        else:
            self.last_mode = "eager"
            self._eager()
        self.mode_counts[self.last_mode] += 1
        return self.loss.loss

    def _key(self, global_batch=None):
        """(batch divisor, collectives on?) -- None: a full batch on every rank -- and, compact="graph", the staged batch's row bucket"""
        key = float(global_batch if global_batch is not None else self.B * self.world), bool(self.comm_enabled)
        return key + (self.rows,) if self.compact_graph else key

    def _captured(self, key):
        """capture the step for ``key`` now unless it is live or the warm-up is not over (True: it is live); what a capture error means"""
        try:
            return self._step_graphs.capture_now(key)
        except RuntimeError as exc:
            # sharded only, and only for errors of the capture mechanism itself (a collective backend that cannot live next to a
            # stream capture): the eager step is the same arithmetic (tests/dist_equiv_worker.py), only with launch overhead.  Any
            # other error -- a failed LB.check, a shape error, out of memory -- is a bug in the captured path and is raised.
            msg = str(exc)
            if not self.sharded or not any(t in msg for t in ("capture", "Capture", "hipErrorStreamCapture", "cudaErrorStreamCapture")):
                raise
            warnings.warn("allrank_amd: hipGraph capture of the sharded step failed (%r); running eagerly" % (exc,))
            self.capture_fallback = repr(exc)                     # queryable: tests/dist_equiv_worker.py asserts it stays None
            self.use_graph = False
            self._graphs.clear()
            return False

    def _warn_evicted(self, key):
        if self._step_graphs.evictions == 1:                      # (say so once)
            if self.compact_graph:
                warnings.warn("allrank_amd: more than %d distinct (batch divisor, row bucket) keys in flight -- evicting the least "
                              "recently used captured step (%d rows); every key beyond the cache costs one re-capture"
                              % (self.max_graphs, key[2]))
                return
            warnings.warn("allrank_amd: more than %d distinct batch divisors in flight -- evicting the least recently used captured "
                          "step (divisor %g); every new divisor costs one re-capture" % (self.max_graphs, key[0]))

    def ensure_captured(self, global_batch=None):
        """Capture the step for this batch divisor NOW -- recording only: nothing executes and no collective is issued -- and say
        whether that worked.  For callers that must agree ACROSS RANKS on captured-vs-eager before any rank runs a step in either form
        (bench.py): each rank calls this after its two eager warm-up steps, the ranks all-reduce the answers, and a rank
        whose peers could not capture switches to eager with them (``use_graph = False``).  It follows ``step()``'s rule.  Before two
        warm-up steps have run it records nothing, returns False and says so in ``capture_fallback`` (``use_graph`` stays on).  After
        them it captures through the same LRU: a full cache evicts its least recently used divisor.  A capture that fails is closed
        (``_capture``) and means what it means in ``step()`` (``_captured``): eager steps for good and False, or the error raised.
        (``step()`` also survives a capture failure of ONE rank: eager and captured steps issue the same collectives in one order.)"""
        if not self.use_graph or self.fcstep:
            return True
        key = self._key(global_batch)
        self._divisor = key[0]
        ok = self._captured(key)
        if not ok and self.use_graph:
            self.capture_fallback = "ensure_captured: not captured -- the two eager warm-up steps have not run yet"
        return ok

    def _fc_step(self, xb, yb, global_batch):
        """the slate-resident step (ltrx_fc_listnet_step): reads the caller's batch in place -- x once -- and leaves scores in
        ``self.scores``, d loss / d scores in ``self.loss.grad`` (with ``keep_loss_grad``), gradients in the flat buffer, the loss in ``self.loss.loss``.  One
        GPU without clipping: the reducing launch also applies Adam (two launches per step); sharded or clipped: gradients only,
        then the all-reduce / clip and the flat-buffer Adam as in the general step."""
        LB = self.LB
        # (the general path's static-buffer copy accepts host batches; so does this one: a host batch is copied to the device first)
        if not xb.is_cuda:
            xb = xb.to(self.dev, non_blocking=True)
        if not yb.is_cuda:
            yb = yb.to(self.dev, non_blocking=True)
        xb = xb.reshape(self.M, -1)
        if xb.dtype != torch.float32 or not xb.is_contiguous():
            xb = xb.float().contiguous()
        if xb.data_ptr() & 15:                                # (the kernel reads 16-byte pieces: a misaligned view is copied once)
            xb = xb.clone()
        yb = yb.reshape(self.B, self.L)
        if yb.dtype != torch.float32 or not yb.is_contiguous():
            yb = yb.float().contiguous()
        LB.require_device(xb, yb)
        self.y_cur = yb
        div = self._key(global_batch)[0]
        fused_adam = not self.sharded and not self.clip
        opt = None
        if fused_adam:
            opt = (self.flat_m, self.flat_v, self.step_count, float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps),
                   self.weight_decay, 1 if self.optimizer == "AdamW" else 0)
        dsc = self.loss.grad if self.keep_loss_grad else None
        H_ = self.fc_sizes[1]
        if self.fcstep == "collapse":
            KN.fc_linear_listnet_step(self.lib, self._st(), xb, yb, self.B, self.L, H_, self.flat_p, *self._fc_offs, self.loss.eps,
                                      self.loss.pad, div, self.scores_raw, self.loss.loss, self.flat_g, self._fc_ws, opt, dsc)
        else:
            KN.fc_listnet_step(self.lib, self._st(), xb, yb, self.B, self.L, H_, self.fc_act, self.flat_p, *self._fc_offs, self.loss.eps,
                               self.loss.pad, div, self.scores_raw, self.loss.loss, self.flat_g, self._fc_ws, opt,
                               self.fc_out[0] if self.keep_fc_out else None, dsc)
        if not fused_adam:
            if self.sharded and self.comm_enabled:
                import torch.distributed as dist
                dist.all_reduce(self.flat_g, op=dist.ReduceOp.SUM, group=self.group)
            self._adam()
        self._images_stale = True                             # (score()'s GEMM forward reads the weight images: refresh them first)
        return self.loss.loss

    def _shard(self, deferred=None):                              # the step's shard context; ``deferred``: see sharding.shard_context
        return sharding.shard_context(int(self._divisor), self.group, deferred=deferred) if self.sharded else contextlib.nullcontext()

    def _eager(self):
        with self._shard():
            self._full()

    @property
    def graph(self):
        """the captured full-batch step (None before capture)"""
        return self._graphs.get(self._key())

    def _capture(self):
        """Record the step as a chain of hipGraph segments.  On one GPU that is a single graph.  Sharded (world > 1), every
        collective of the step -- the bucketed gradient all-reduces, the wait before Adam, and the one-float all-reduce of a
        batch-global loss normaliser (sharding.allreduce_sum_) -- ends the segment being recorded and is kept as the host
        action to run between two replays: the compute of a step is ~75 launches of 10-300 us at 64 slates per GPU (launch
        latency matters exactly where 8-GPU runs sit), while the collectives stay ordinary torch.distributed calls on the
        process group's stream, whatever the backend (RCCL on a node, gloo in the one-GPU tests).
        The cyclic collector rests meanwhile (``_collector_at_rest``)."""
        with _collector_at_rest():
            return self._record_step()

    def _record_step(self):
        if self._cap_stream is None:
            self._cap_stream = torch.cuda.Stream(device=self.dev)
        segs = []
        torch.cuda.synchronize(self.dev)
        self._cap_stream.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self._cap_stream):
            # "thread_local": only this thread's calls are checked against the capture -- a process group's watchdog thread or a
            # data-loader thread touching the runtime must not invalidate it
            cur = [torch.cuda.CUDAGraph()]
            cur[0].capture_begin(pool=self._step_graphs.pool, capture_error_mode="thread_local")

            def seg_break(after):
                cur[0].capture_end()
                segs.append((cur[0], after))
                cur[0] = torch.cuda.CUDAGraph()
                cur[0].capture_begin(pool=self._step_graphs.pool, capture_error_mode="thread_local")

            self._seg_break = seg_break
            ok = False
            try:
                with self._shard(deferred=seg_break):
                    self._full()
                ok = True
            finally:
                self._seg_break = None
                try:
                    cur[0].capture_end()
                except Exception:                     # noqa: BLE001 -- the original error (if any) is the one to report
                    if ok:
                        raise
            segs.append((cur[0], None))
        torch.cuda.current_stream(self.dev).wait_stream(self._cap_stream)
        return segs

    def score(self, xb, yb, indices=None, lengths=None):
        """``model.score(xb, yb == PADDED_Y_VALUE, indices)`` in eval mode (model.py:82-92) through the kernels of the training
        step -- the forward half only, every dropout off, replayed from its own hipGraph -- for the validation / metric passes of
        an epoch (train_utils.py:32-56, 101-107).  The nn.Module forward computes the same scores with fp32 library GEMMs at
        less than half the rate.  ``yb`` only provides the padding mask; the batch must have the trainer's [B, L] shape
        (``pad_batch``) and is staged as ``step()`` stages it.  Returns the trainer's ``scores`` [B, L] (valid until the next call)."""
        self._reattach()
        self._sync_weights()
        self._stage_batch(xb, yb, indices, lengths, "score")
        if self.use_graph and self.layout != "cu":                # (compact="graph": the row count varies, the one-key cache does not
            #                                                        fit; the forward runs eagerly -- FusedScorer is the captured one)
            self._fwd_graphs.run(0, lambda: self._forward(False))
        else:
            self._forward(False)
        return self.scores

    def score_block(self, xb, yb, indices, lengths=None):
        """``score`` for a validation block of n <= B slates of the training slate length, topped up as ``step_block`` does: (scores
        [n, L], the model output and the labels of max(n, 1) slates for the loss -- an empty shard still enters it, with one fully
        padded slate), or None for a block of another shape"""
        n = int(xb.shape[0])
        if n > self.B or tuple(xb.shape[1:2]) != (self.L,):
            return None
        xs, ys, ids, lengths = self._block(xb, yb, indices, lengths)
        return self.score(xs, ys, ids, lengths=lengths)[:n], self.scores_raw[:max(n, 1)], ys[:max(n, 1)]

    def scorer(self, B, L, use_graph=True, max_graphs=8):
        """a FusedScorer for validation batches of ``B`` slates padded to ``L`` items (any L up to LTRX_MAX_METRIC_SLATE_LEN)"""
        return FusedScorer(self, B, L, use_graph=use_graph, max_graphs=max_graphs)


class FusedScorer(object):
    """``model.eval(); model.score(...)`` for batches of up to ``B`` slates padded to ``L`` items -- the validation shape, where the
    reference pads every slate to the longest one of the set (dataset_loading.py:185-194) -- through the forward kernels of a
    FusedTrainer (``FusedTrainer._forward`` over this object's buffers), on the VALID rows only:

      * the batch's valid items are packed into consecutive rows (``run_resident``: straight from the resident CSR set,
        ltrx_assemble_packed -- the padded [B, L, F] features are never written; ``run``: gathered from a padded batch,
        ltrx_gather_rows_cu), attention runs per slate from cu_seqlens, and the packed scores go back to the padded grid with 0 on
        padded slots (ltrx_scatter_rows_cu) -- the value compact training leaves there;
      * the weights are the trainer's (flat parameters, weight images and transposes), re-synced before every call as ``score()``
        does, so every optimizer step is seen;
      * nothing is saved for a backward: the ``saved=False`` buffer set of ``_alloc_forward`` (bytes: ``self.nbytes``);
      * the row count is rounded up the ladder of ``row_bucket``, and the bucket keys the forward-graph rule of ``_GraphLRU`` (LRU of
        ``max_graphs`` buckets) -- the kernels read the valid-row count from device memory, so a graph is right for every batch of
        its bucket;
      * per batch the host only picks the bucket from the host lengths and uploads prefix sums, launch order and slate ids
        (``_Stager``): no host sync.  ``run`` without host lengths counts the valid items on the device -- one sync, as compact
        training does.
    Results (``scores_raw`` [B, L] or [B, L, d_output], ``scores`` [B, L], labels ``y`` [B, L] of ``run_resident``) stay valid until
    the next call.  ``packed()`` gives the same batch in the ragged layout of allrank_amd.ragged -- the packed scores the forward
    wrote (before the scatter), the packed labels, ``cu``, ``order`` and the batch's host ``max_len`` -- for a loss and metrics that
    run on the valid items only."""

    def __init__(self, trainer, B, L, use_graph=True, max_graphs=8):
        from . import _lib as LB
        t = trainer
        B, L = int(B), int(L)
        if B <= 0 or L <= 0:
            raise ValueError("FusedScorer: B and L must be positive")
        if L > LB.MAX_METRIC_SLATE_LEN:
            raise ValueError("FusedScorer: slate length %d above LTRX_MAX_METRIC_SLATE_LEN = %d" % (L, LB.MAX_METRIC_SLATE_LEN))
        self.t, self.LB = t, LB
        self.cap = (B * L + 31) // 32 * 32                 # the largest rung: every slot of the batch valid
        _alloc_forward(self, t, self.cap, B, L, saved=False, layout="cu")
        self.ids = self._stager.ids
        self.rows, self.n_valid = 32, 0
        self.y = torch.full((B, L), float(PADDED_Y_VALUE), dtype=torch.float32, device=t.dev)
        self.y_c = torch.zeros(self.cap, dtype=torch.float32, device=t.dev)     # the labels of the packed rows (``packed()``)
        self.max_len, self._y_c_fresh = 0, False           # longest slate of the last batch (host); y_c holds that batch's labels
        seen, nb = set(), 0
        for v in list(vars(self).values()) + [v for st in self.layers for v in st.values()]:
            if torch.is_tensor(v) and v.is_cuda and v.untyped_storage().data_ptr() not in seen:
                seen.add(v.untyped_storage().data_ptr())
                nb += v.untyped_storage().nbytes()
        self.nbytes = nb
        self.use_graph, self.max_graphs = bool(use_graph), int(max_graphs)
        self._fwd_graphs = _GraphLRU(max_graphs, new_pool=torch.cuda.graph_pool_handle)
        self._graphs = self._fwd_graphs.graphs             # row bucket -> captured forward, least recently used first
        self.last_mode, self.evictions = None, 0           # "eager" / "capture" / "replay" of the last call; buckets evicted so far

    def _host_lengths(self, lengths):
        """host lengths of one batch, range-checked, as the int32 tensor the stager uploads; keeps the batch's ``max_len``"""
        lens = torch.as_tensor(lengths, dtype=torch.int32).reshape(-1)
        n = int(lens.numel())
        if n > self.B:
            raise ValueError("FusedScorer: %d slates in a batch of a %d-slate scorer" % (n, self.B))
        if n and int(lens.max()) > self.L:
            raise ValueError("FusedScorer: a slate of %d items in a scorer for slate length %d" % (int(lens.max()), self.L))
        self.max_len = max(int(lens.max()), 0) if n else 0
        return lens.clamp(min=0)

    def _sync(self):
        self.t._reattach()
        self.t._sync_weights()

    def run_resident(self, slates, ids, lengths, position=None):
        """scores of the slates ``ids`` (host int64, at most B) of the resident set ``slates`` (a data.DeviceSlates) padded to L;
        ``lengths``: their item counts (host; every one <= L -- the padding branch of FixLength).  Also fills ``self.y`` with the
        padded labels.  ``position`` (an int; None: every item's index in its slate): the position a positional encoding sees for
        EVERY item -- the reference's inference feeds ones (inference_utils.py:47).  Returns ``scores_raw``."""
        t, LB = self.t, self.LB
        ids_h = torch.as_tensor(ids, dtype=torch.int64).cpu().reshape(-1)
        if ids_h.numel() and (int(ids_h.min()) < 0 or int(ids_h.max()) >= slates.n_slates):
            raise ValueError("FusedScorer.run_resident: slate id outside the set")
        if slates.n_features != t.fc_sizes[0]:
            raise ValueError("FusedScorer.run_resident: %d features, the model takes %d" % (slates.n_features, t.fc_sizes[0]))
        LB.require_device(slates.x_items)
        self._sync()
        RW.set_rows(self, self._stager.upload(self._host_lengths(lengths), ids_h))     # cu_seqlens, launch order, ids: no host sync
        KN.assemble_packed(t.lib, t._st(), slates.x_items, slates.y_items, slates.offsets, self.ids, self.cu, self.B, self.L, self.rows,
                           self.x_in, self.y, self.idx, self.idx_rows if t.pos is not None else None)
        if position is not None and t.pos is not None:
            self.idx_rows[:self.n_valid].fill_(int(position))     # (the alignment rows keep the padding position -1)
        self._run()
        return self.scores_raw

    def run(self, xb, yb, indices=None, lengths=None):
        """scores of a padded batch ``xb`` [n, L, F] (n <= B; valid items first in every slate, labels ``yb`` == -1 on padding, as
        dataset.py:28-38 pads); ``lengths``: host item counts per slate (None: counted on the device, one host sync).  Returns
        ``scores_raw``."""
        t, B, L = self.t, self.B, self.L
        n_sl = int(xb.shape[0])
        if n_sl > B or int(xb.shape[1]) != L:
            raise ValueError("FusedScorer.run: batch %s, scorer for %d slates of %d items" % (tuple(xb.shape), B, L))
        if t.pos is not None and indices is None:
            raise ValueError("FusedScorer.run: the model has a positional encoding, run() needs `indices`")
        xb = xb.to(t.dev, torch.float32).contiguous()
        yb = yb.to(t.dev, torch.float32)
        self._sync()
        self.y[:n_sl].copy_(yb)
        self.y[n_sl:].fill_(float(PADDED_Y_VALUE))
        lens = self._host_lengths(lengths) if lengths is not None else None
        got = RW.stage_cu(self, t.lib, t._st(), xb, indices if t.pos is not None else None, lens,
                          valid=None if lens is not None else yb != PADDED_Y_VALUE, want=("n", "max_len"))
        self.max_len = got.get("max_len", self.max_len)    # (host lengths: _host_lengths has set it)
        self._run()
        return self.scores_raw

    def packed(self):
        """The last batch in the ragged layout (include/ltrx.h): (scores [n], labels [n], cu_seqlens [B+1], launch order [B], host
        max_len).  The scores are the rows the forward wrote before scattering them (d_output == 1), the labels are packed from
        ``self.y`` on the first call after a run; both stay valid until the next run."""
        if self.t.n_out != 1:
            raise NotImplementedError("FusedScorer.packed: d_output > 1 (the ordinal loss reads the padded grid)")
        if not self._y_c_fresh:
            KN.gather_rows_cu(self.t.lib, self.t._st(), self.y, self.cu, self.B, self.L, 1, self.rows, self.y_c, None, "gather_rows_cu(labels)")
            self._y_c_fresh = True
        n = self.n_valid
        return self.scores_c[:n], self.y_c[:n], self.cu, self.order, self.max_len

    def _run(self):
        self._y_c_fresh = False
        fwd = lambda: self.t._forward(False, self)
        if self.use_graph:
            self.last_mode = self._fwd_graphs.run(self.rows, fwd)
            self.evictions = self._fwd_graphs.evictions
        else:
            self.last_mode = "eager"
            fwd()


# ------------------------------------------------------------------------------------------------------------------
# epoch loop on device-resident data  (the body of fit(), allrank/training/train_utils.py:78-147, without its host work)
# ------------------------------------------------------------------------------------------------------------------
def fit_device(model, loss_name, loss_args, train_ds, val_ds, epochs, batch_size, slate_length, metrics=None, lr=1e-3,
               val_metric=None, early_stopping_patience=None, generator=None, use_fused=True, log=None,
               gradient_clipping_norm=None, lr_schedule=None, compact=False):
    """Train ``model`` on a DeviceSlates dataset; returns {"epochs", "train_loss", "val_metrics", "history"}.

    Per epoch: shuffled batches produced on the device (DeviceSlates.batches), one training step each (FusedTrainer when
    the model family / dropout allow it, else the autograd Trainer), the running loss is accumulated ON THE DEVICE (one
    host sync per epoch instead of the reference's ``loss.item()`` per step, train_utils.py:29), then one no-grad
    metrics pass over the validation set (train_utils.py:101-107).  The reference's second full pass over the TRAIN set
    for train metrics (train_utils.py:99, in train() mode, i.e. dropout active) is replaced by metrics taken from the
    scores of the TRAINING forward itself (same mode, no extra model pass): ``train_<metric>_<k>`` in
    the history is the mean over the epoch's training batches, each evaluated with the weights it was scored with.
    ``gradient_clipping_norm``: train_utils.py:24-25; ``lr_schedule(epoch) -> lr`` plays the role of the per-epoch
    ``scheduler.step()`` (train_utils.py:117-118), e.g. ``lambda e: 1e-3 * 0.1 ** (e // 50)`` for StepLR(50, 0.1).
    ``compact=True`` runs the fused step over the valid items only (FusedTrainer(compact=True))."""
    from . import losses as E
    from . import metrics as EMx
    from .data import evaluate
    metrics = metrics or {"ndcg": [5]}
    trainer, fused = None, False
    if use_fused:
        try:
            trainer = FusedTrainer(model, loss_name, loss_args, batch_size, slate_length, lr=lr, use_graph=True,
                                   gradient_clipping_norm=gradient_clipping_norm, compact=compact)
            fused = True
        except NotImplementedError:
            trainer = None
    if trainer is None:
        lossfn = (lambda s, t: getattr(E, loss_name)(s, t, **(loss_args or {})))
        trainer = Trainer(model, lossfn, torch.optim.Adam(model.parameters(), lr=lr), gradient_clipping_norm)
    history, best, best_epoch = [], -1.0, 0
    if epochs <= 0:
        return dict(epochs=0, train_loss=float("nan"), val_metrics=evaluate(model, val_ds, metrics), history=[], fused=fused)
    for epoch in range(epochs):
        if lr_schedule is not None:
            new_lr = float(lr_schedule(epoch))
            if fused:
                trainer.set_lr(new_lr)
            else:
                for g_ in trainer.opt.param_groups:
                    g_["lr"] = new_lr
        model.train()
        tot = torch.zeros(1, device=train_ds.device)
        nb = 0
        tm = {name: None for name in metrics} if fused else {}
        for xb, yb, idx in train_ds.batches(batch_size, slate_length, shuffle=True, generator=generator, drop_last=False):
            real = xb.shape[0]
            if fused and real < batch_size:
                # the last batch of an epoch (DataLoader drop_last=False, dataset_loading.py:245): the fused step has static
                # shapes, so the batch is topped up with fully padded slates (label -1, features 0: no loss, no gradient) and
                # the loss is normalised by the REAL slate count, exactly what the reference computes on the short batch
                xb, yb, idx = pad_batch(xb, yb, idx, batch_size)
                loss = trainer.step(xb, yb, idx, global_batch=real)
            else:
                loss = trainer.step(xb, yb, idx)
            tot += loss.detach().view(1) * real
            nb += real
            for name in tm:                                   # metrics of the training forward (scores of this very step)
                v = getattr(EMx, name)(trainer.scores[:real], trainer.y_cur[:real], ats=metrics[name]).sum(0)
                tm[name] = v if tm[name] is None else tm[name] + v
        train_loss = float(tot.item()) / max(nb, 1)
        val = evaluate(model, val_ds, metrics)
        rec = dict(epoch=epoch, train_loss=train_loss, **val)
        for name, v in tm.items():
            if v is not None:
                for at, x_ in zip(metrics[name], (v / max(nb, 1)).cpu().numpy()):
                    rec["train_%s_%d" % (name, at)] = float(x_)
        history.append(rec)
        if log:
            log(history[-1])
        if val_metric is not None and early_stopping_patience is not None:
            cur = val[val_metric]
            if cur > best:
                best, best_epoch = cur, epoch
            if epoch - best_epoch > early_stopping_patience:       # early_stop.py:17-19
                break
    return dict(epochs=epoch, train_loss=history[-1]["train_loss"], val_metrics={k: v for k, v in history[-1].items()
                                                                                 if k not in ("epoch", "train_loss")
                                                                                 and not k.startswith("train_")},
                history=history, fused=fused)
