"""Record which libltrx calls the package makes, and what they compute, over a set of small cases (needs the MI355X).

    python tests/golden/make_call_trace_fixture.py [--set calls|rows|step|options|fit] [--out FILE] [--commit HASH]

Five case sets, one file each, each run ONCE at the commit named in its file ("commit"):
  calls  tests/golden/call_trace_parent.json: before the GEMM, attention, LayerNorm and head calls of allrank_amd/ops.py and
         allrank_amd/engine.py moved into the launchers of allrank_amd/kernels.py;
  rows   tests/golden/call_trace_rows_parent.json: the three row layouts (padded grid, index-packed, cu_seqlens-packed) before their
         staging and row movers moved into allrank_amd/rows.py and the packing launchers of allrank_amd/kernels.py;
  step   tests/golden/call_trace_step_parent.json: what the two sets above do not reach, before the training step's own calls, the
         ranking call and the click call moved into allrank_amd/kernels.py -- the slate-resident FC + ListNet step (with Adam in the
         launch, with the separate clip + Adam launches, and the linear-scorer form), SGD with Nesterov momentum and without a
         momentum buffer, ``first_nonfinite``, ``inference.rank_batches`` from a padded batch and from a resident set, and
         ``clicks.click_on_slates`` with a cascade and a diverse plan;
  options tests/golden/call_trace_options_parent.json: before the step's operands (parameter views, transposed copies, weight images)
         became records built once at construction -- each A/B switch of the large-tile step off on its own, the two-group
         weight-gradient composition under sublayer dropout, an FC stack of three layers, the fixed positional encoding on the
         padded grid, ``score()`` between two steps, ``load_state_dict`` with another seed, and a scorer over an ``input_norm`` model
         with 46 features.  Its traces begin at the constructor: the size and support queries made there are held too.
  fit    tests/golden/call_trace_fit_parent.json: before the two engines shared one interface under ``fit()`` -- whole ``fit()`` calls
         (hipGraph capture on, as a user runs them) over a small libsvm set written here: both engines, the four validation score
         sources, the ragged evaluation, schedulers, early stopping, the finiteness check, checkpoint and resume.  Per case the
         trace of the whole call, digests of the result, ``last_run``, the validation losses, ``model.pkl`` and the checkpoint, and
         ``notes``: plain facts (engine, batches per score source, the error text) that the two runs must agree on as well.
tests/test_gpu_call_trace.py runs the same cases at every later commit and holds them to the recorded calls and results exactly.
Re-running a set at a later commit only re-records that commit against itself.

Only public entry points are used (FusedTrainer, FusedScorer, allrank_amd.ops, inference.rank_batches, clicks.click_on_slates).  The object ``allrank_amd._lib.lib()`` caches is
replaced by a proxy before anything is constructed; while a case records, the proxy logs every call as ``[name, [arguments]]``:
an argument whose type in ``_lib.SIGNATURES`` is a pointer (the stream included) as 0 or 1 -- NULL or not -- and integers and floats
as they are.  Per trainer case: the trace of the first step (``use_graph=False``: every step makes its calls) and SHA-256 digests of the raw
bytes of the loss of each of 3 steps, the flat gradient after step 1, the flat parameters after step 3 and the scores.  Every case
runs twice; a digest is stored only where the two runs agree bit for bit (``unstable`` names the others), and the two traces must
be equal.  ``gemm="hipblaslt"`` is recorded without digests: torch's GEMMs choose their own algorithm.
"""
import atexit
import contextlib
import ctypes
import functools
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
FIXTURE = os.path.join(HERE, "call_trace_parent.json")
ROWS_FIXTURE = os.path.join(HERE, "call_trace_rows_parent.json")
STEP_FIXTURE = os.path.join(HERE, "call_trace_step_parent.json")
OPTIONS_FIXTURE = os.path.join(HERE, "call_trace_options_parent.json")
FIT_FIXTURE = os.path.join(HERE, "call_trace_fit_parent.json")


# ------------------------------------------------------------------------------------------------------------------
# the recording proxy
# ------------------------------------------------------------------------------------------------------------------
class _Proxy(object):
    """stands where ``_lib.lib()`` keeps the bound library: passes every call on, logs it while ``log`` is a list"""

    def __init__(self, real, signatures):
        self._real, self._sig, self.log = real, signatures, None

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        types = self._sig[name][1]

        def call(*args):
            if self.log is not None:
                self.log.append([name, [_plain(a, t) for a, t in zip(args, types)]])
            return fn(*args)
        return call


def _plain(a, ctype):
    if ctype is ctypes.c_void_p:                               # any pointer or the stream: NULL or not
        if a is None:
            return 0
        if isinstance(a, ctypes.c_void_p):
            return int(bool(a.value))
        return int(bool(a)) if isinstance(a, int) else 1        # (arrays and byref() objects are never NULL)
    a = getattr(a, "value", a)                                 # a ctypes scalar
    return float(a) if ctype is ctypes.c_float else int(a)


@contextlib.contextmanager
def proxied():
    """the proxy in place of the cached library object for the enclosed region"""
    from allrank_amd import _lib
    real = _lib.lib()
    proxy = _Proxy(real, _lib.SIGNATURES)
    _lib._lib = proxy
    try:
        yield proxy
    finally:
        _lib._lib = real


@contextlib.contextmanager
def _recording(proxy, trace):
    proxy.log = trace
    try:
        yield
    finally:
        proxy.log = None


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------------------
# models and batches
# ------------------------------------------------------------------------------------------------------------------
def _model(F, sizes, N=0, d_ff=64, h=4, dropout=0.0, pe=None, input_norm=False, act=None, fc_dropout=0.0, out_act=None, d_output=1):
    from allrank_amd.model import make_model
    torch.manual_seed(11)
    tr = dict(N=N, d_ff=d_ff, h=h, positional_encoding=pe, dropout=dropout) if N else None
    return make_model(dict(sizes=list(sizes), input_norm=input_norm, activation=act, dropout=fc_dropout), tr,
                      dict(d_output=d_output, output_activation=out_act), F).to(DEV)


def _batch(lens, L, F, seed):
    """padded batch (valid items first; features 0, label -1, index -1 on padding) with the given slate lengths"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    x = rng.standard_normal((n, L, F)).astype(np.float32)
    y = rng.integers(0, 5, (n, L)).astype(np.float32)
    idx = np.tile(np.arange(L, dtype=np.int64), (n, 1))
    for b, k in enumerate(lens):
        x[b, k:], y[b, k:], idx[b, k:] = 0, -1, -1
    return (torch.tensor(x, device=DEV), torch.tensor(y, device=DEV), torch.tensor(idx, device=DEV),
            torch.tensor(np.asarray(lens, dtype=np.int32)))


SMALL = dict(F=20, sizes=[32], N=2, d_ff=64, h=4, dropout=0.1)               # the small-tile encoder, B 5, L 70
SMALL_LENS = [70, 31, 70, 8, 55]
LARGE = dict(F=136, sizes=[256], N=1, d_ff=512, h=4)                         # head width 64, 2048 rows: the large-tile arms
LARGE_LENS = [128] * 12 + [100, 128, 77, 128]
LARGE_RAGGED = [128, 90, 3, 128, 61, 128, 17, 128, 128, 45, 128, 99, 128, 128, 1, 110]


def _train(proxy, model_kw, loss, largs, lens, L, use_idx=False, host_lengths=False, digests=True, construct=False, **trainer_kw):
    """``construct``: the trace begins with the calls the constructor makes (size and support queries, the first image refresh)"""
    from allrank_amd.engine import FusedTrainer
    model = _model(**model_kw)
    trace, dig = [], {}
    with _recording(proxy, trace if construct else None):
        ft = FusedTrainer(model, loss, largs, len(lens), L, use_graph=False, seed=1234, **trainer_kw)
    x, y, idx, hl = _batch(lens, L, model_kw["F"], 3)
    kw = dict(indices=idx) if use_idx else {}
    if host_lengths:
        kw["lengths"] = hl
    for s in range(3):
        with _recording(proxy, trace if s == 0 else None):
            loss_t = ft.step(x, y, **kw)
        dig["loss%d" % (s + 1)] = _sha(loss_t)
        if s == 0:
            dig["flat_g"] = _sha(ft.flat_g)
    dig["flat_p"], dig["scores"] = _sha(ft.flat_p), _sha(ft.scores)
    return trace, (dig if digests else {})


def _score(proxy):
    from allrank_amd.engine import FusedTrainer
    ft = FusedTrainer(_model(**SMALL), "listNet", {}, 5, 70, use_graph=False, seed=1234)
    x, y, _, _ = _batch(SMALL_LENS, 70, 20, 3)
    ft.step(x, y)
    trace = []
    with _recording(proxy, trace):
        sc = ft.score(x, y)
    return trace, dict(scores=_sha(sc))


SCORER_LENS = [90, 1, 44, 0, 59]


def _pe_trainer():
    """the SMALL encoder with a fixed positional encoding, one step taken"""
    from allrank_amd.engine import FusedTrainer
    ft = FusedTrainer(_model(pe=dict(strategy="fixed", max_indices=100), **SMALL), "listNet", {}, 5, 70, use_graph=False, seed=1234)
    xt, yt, it, _ = _batch(SMALL_LENS, 70, 20, 3)
    ft.step(xt, yt, it)
    return ft


def _packed_digests(sc, raw):
    ps, py, cu, order, max_len = sc.packed()
    return dict(scores=_sha(raw), packed_scores=_sha(ps), packed_labels=_sha(py), cu=_sha(cu), order=_sha(order))


def _scorer(proxy, lens=SCORER_LENS, host_lengths=True):
    sc = _pe_trainer().scorer(5, 90, use_graph=False)
    x, y, idx, hl = _batch(lens, 90, 20, 4)
    trace = []
    with _recording(proxy, trace):
        raw = sc.run(x, y, idx, lengths=hl if host_lengths else None)
        dig = _packed_digests(sc, raw)
    return trace, dig


def _scorer_resident(proxy):
    from allrank_amd.data import DeviceSlates
    lens = [9, 1, 30, 0 + 1, 17, 30]
    rng = np.random.default_rng(6)
    X = rng.standard_normal((sum(lens), 20)).astype(np.float32)
    y = rng.integers(0, 5, sum(lens)).astype(np.float32)
    ds = DeviceSlates(X, y, np.repeat(np.arange(len(lens)), lens), device=DEV)
    sc = _pe_trainer().scorer(4, 30, use_graph=False)
    ids = [5, 0, 2]
    trace = []
    with _recording(proxy, trace):
        raw = sc.run_resident(ds, torch.tensor(ids, dtype=torch.int64), torch.tensor([lens[i] for i in ids], dtype=torch.int32))
        dig = dict(_packed_digests(sc, raw), y=_sha(sc.y))
    return trace, dig


def _ops(fn):
    """an ops case: ``fn(rng)`` -> (inputs that take a gradient, a function of them); forward and backward are both recorded"""
    def run(proxy):
        rng = np.random.default_rng(5)
        leaves, f = fn(lambda *shape: torch.tensor(rng.standard_normal(shape).astype(np.float32), device=DEV))
        for t in leaves:
            t.requires_grad_(True)
        trace = []
        with _recording(proxy, trace):
            out = f(*leaves)
            outs = [o for o in (out if isinstance(out, tuple) else (out,)) if o is not None]
            torch.manual_seed(3)
            torch.autograd.backward(outs, [torch.randn(o.shape, device="cpu").to(DEV) for o in outs])
        dig = {"out%d" % i: _sha(o) for i, o in enumerate(outs)}
        dig.update({"grad%d" % i: _sha(t.grad) for i, t in enumerate(leaves)})
        return trace, dig
    return run


def _key_mask(B, L, lens):
    m = torch.zeros((B, L), dtype=torch.bool, device=DEV)
    for b, k in enumerate(lens):
        m[b, k:] = True
    return m


def _op_cases():
    from allrank_amd import ops
    B, L, d, h = 3, 50, 32, 4
    mask = lambda: _key_mask(B, L, [50, 17, 33])  # noqa: E731
    return {
        "ops.linear": _ops(lambda r: ((r(B, L, 36), r(52, 36), r(52)), lambda x, w, b: ops.linear(x, w, b, 0))),
        "ops.linear_relu": _ops(lambda r: ((r(B, L, 36), r(52, 36), r(52)), lambda x, w, b: ops.linear(x, w, b, 1))),
        "ops.feed_forward": _ops(lambda r: ((r(B, L, 36), r(64, 36), r(64), r(36, 64), r(36)),
                                            lambda x, w1, b1, w2, b2: ops.feed_forward(x, w1, b1, w2, b2, 0.2, seed=77))),
        "ops.layer_norm": _ops(lambda r: ((r(B, L, 40), r(40), r(40)), lambda x, a, b: ops.layer_norm(x, a, b))),
        "ops.layer_norm_residual": _ops(lambda r: ((r(B, L, 40), r(B, L, 40), r(40), r(40)),
                                                   lambda x, res, a, b: ops.layer_norm_residual(x, res, a, b))),
        "ops.attention": _ops(lambda r: ((r(B, L, 3 * d),), lambda qkv: ops.attention(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:],
                                                                                      mask(), h, 0.1, seed=5))),
        "ops.attention_packed": _ops(lambda r: ((r(B, L, 3 * d),), lambda qkv: ops.attention_packed(qkv, mask(), h, 0.1, seed=5))),
        "ops.score_head": _ops(lambda r: ((r(B, L, 40), r(1, 40), r(1)), lambda x, w, b: ops.score_head(x, w, b))),
    }


def cases():
    """{name: run(proxy) -> (trace, digests)}"""
    fc46 = dict(F=46, sizes=[64, 32], input_norm=True, act="ReLU", fc_dropout=0.2)
    fc_tanh = dict(F=24, sizes=[48, 32], act="Tanh", out_act="Sigmoid")
    pe = dict(SMALL, pe=dict(strategy="learned", max_indices=100), d_output=4, out_act="Sigmoid")
    large_drop = dict(LARGE, dropout=0.1)
    out = {
        "small_encoder": lambda p: _train(p, SMALL, "listNet", {}, SMALL_LENS, 70),
        "large_tile": lambda p: _train(p, LARGE, "approxNDCGLoss", {}, LARGE_LENS, 128),
        # 8 x 21 = 168 tiles of 256 x 256 in the feed-forward GEMMs: where ltrx_gemm_nt_relu_bits_bytes grants the one-bit ReLU mask
        "large_tile_relu_bits": lambda p: _train(p, dict(LARGE, d_ff=5376, dropout=0.1), "approxNDCGLoss", {}, LARGE_LENS, 128),
        "large_tile_compact_host_lengths": lambda p: _train(p, large_drop, "approxNDCGLoss", {}, LARGE_RAGGED, 128, host_lengths=True,
                                                            compact=True),
        "large_tile_compact_device_count": lambda p: _train(p, large_drop, "approxNDCGLoss", {}, LARGE_RAGGED, 128, compact=True),
        "fc_input_norm_46": lambda p: _train(p, fc46, "listNet", {}, [30, 12, 30, 1], 30),
        "fc_tanh_sigmoid": lambda p: _train(p, fc_tanh, "listNet", {}, [30, 12, 30, 1], 30),
        "learned_pe_ordinal_clip_adamw": lambda p: _train(p, pe, "ordinal", {"n": 4}, SMALL_LENS, 70, use_idx=True,
                                                          gradient_clipping_norm=0.5, optimizer="AdamW", weight_decay=0.01),
        "sgd_momentum": lambda p: _train(p, SMALL, "listNet", {}, SMALL_LENS, 70, optimizer="SGD", momentum=0.9, lr=0.01),
        "gemm_split_bf16_strict": lambda p: _train(p, SMALL, "listNet", {}, SMALL_LENS, 70, gemm="split_bf16_strict"),
        "gemm_bf16": lambda p: _train(p, SMALL, "listNet", {}, SMALL_LENS, 70, gemm="bf16"),
        "gemm_hipblaslt": lambda p: _train(p, SMALL, "listNet", {}, SMALL_LENS, 70, gemm="hipblaslt", digests=False),
        "score": _score,
        "scorer_run_packed": _scorer,
    }
    out.update(_op_cases())
    return out


def rows_cases():
    """the second set: the cu_seqlens layout of the trainer (compact="graph") and of the scorer, the index layout's positions"""
    pe = dict(SMALL, pe=dict(strategy="fixed", max_indices=100))
    return {
        "compact_graph_host_lengths": lambda p: _train(p, SMALL, "listNet", {}, SMALL_LENS, 70, host_lengths=True, compact="graph"),
        "compact_graph_device_count": lambda p: _train(p, SMALL, "listNet", {}, SMALL_LENS, 70, compact="graph"),
        "compact_graph_pe": lambda p: _train(p, pe, "listNet", {}, SMALL_LENS, 70, use_idx=True, host_lengths=True, compact="graph"),
        "compact_index_pe": lambda p: _train(p, pe, "listNet", {}, SMALL_LENS, 70, use_idx=True, host_lengths=True, compact=True),
        "scorer_run_device_count": lambda p: _scorer(p, host_lengths=False),
        "scorer_run_short_batch": lambda p: _scorer(p, lens=SCORER_LENS[:3]),
        "scorer_run_resident": _scorer_resident,
    }


FC_STEP = dict(F=20, sizes=[16], act="ReLU")                                 # B 6, L 16: the slate-resident FC + ListNet step
FC_LENS = [16, 8, 1, 0, 15, 3]
RANK_LENS = [70, 1, 33, 12]


def _sha_bytes(b):
    return hashlib.sha256(b).hexdigest()


def _first_nonfinite(proxy):
    from allrank_amd.engine import FusedTrainer
    ft = FusedTrainer(_model(**SMALL), "listNet", {}, 5, 70, use_graph=False, seed=1234)
    x, y, _, _ = _batch(SMALL_LENS, 70, 20, 3)
    ft.step(x, y)
    trace = []
    with _recording(proxy, trace):
        found = ft.first_nonfinite()
    return trace, dict(flat_g=_sha(ft.flat_g), found=_sha_bytes(repr(found).encode()))


def _rank_batches(resident):
    def run(proxy):
        from allrank_amd import inference
        from allrank_amd.data import DeviceSlates
        model = _model(**dict(SMALL, dropout=0.0))
        x, y, _, hl = _batch(RANK_LENS, 70, 20, 8)
        if resident:
            valid = (y != -1).cpu().numpy()
            ds = DeviceSlates(x.cpu().numpy()[valid], y.cpu().numpy()[valid], np.repeat(np.arange(len(RANK_LENS)), RANK_LENS), device=DEV)
            batch = (ds, torch.arange(len(RANK_LENS), dtype=torch.int64), hl)
        else:
            batch = (x, y)
        trace = []
        with _recording(proxy, trace):
            (xr, yr), = list(inference.rank_batches(model, [batch], len(RANK_LENS), 70))
            dig = dict(x_ranked=_sha(xr), y_ranked=_sha(yr))
        assert inference.last_run["engine"] == "fused", inference.last_run
        return trace, dig
    return run


def _clicks(case):
    def run(proxy):
        from allrank_amd import clicks
        from tests import click_cases as CC
        X, y = CC.inputs(case)
        rows = [1, 4, 6, 9]                                    # 4 slates: 1, 4, 13 and 65 items
        np.random.seed(CC.CASES[case]["seed"])
        trace = []
        with _recording(proxy, trace):
            _, got = clicks.click_on_slates((torch.tensor(X[rows], device=DEV), torch.tensor(y[rows], device=DEV)),
                                            CC.ours(CC.CASES[case]["model"]), include_empty=True)
        assert clicks.last_run["engine"] == "device", clicks.last_run
        return trace, dict(clicks=_sha_bytes(np.stack(got).tobytes()))
    return run


def step_cases():
    """the third set: the step's own calls that the first two sets do not reach, ranking and clicks"""
    sgd = dict(optimizer="SGD", lr=0.01)
    return {
        "fc_listnet_step": lambda p: _train(p, FC_STEP, "listNet", {}, FC_LENS, 16),
        "fc_listnet_step_clip": lambda p: _train(p, FC_STEP, "listNet", {}, FC_LENS, 16, gradient_clipping_norm=0.05),
        "fc_linear_listnet_step": lambda p: _train(p, dict(FC_STEP, act=None), "listNet", {}, FC_LENS, 16, fc_step="collapse"),
        "sgd_nesterov_weight_decay": lambda p: _train(p, SMALL, "listNet", {}, SMALL_LENS, 70, momentum=0.9, nesterov=True,
                                                      weight_decay=0.01, **sgd),
        "sgd_no_momentum": lambda p: _train(p, SMALL, "listNet", {}, SMALL_LENS, 70, momentum=0.0, **sgd),
        "first_nonfinite": _first_nonfinite,
        "rank_batches_grid": _rank_batches(False),
        "rank_batches_resident": _rank_batches(True),
        "click_on_slates_cascade": _clicks("plain.cascade"),
        "click_on_slates_diverse": _clicks("shipped.lattice.F3"),
    }


def _step_score_step(proxy):
    from allrank_amd.engine import FusedTrainer
    trace, dig = [], {}
    with _recording(proxy, trace):
        ft = FusedTrainer(_model(**SMALL), "listNet", {}, 5, 70, use_graph=False, seed=1234)
        x, y, _, _ = _batch(SMALL_LENS, 70, 20, 3)
        dig["loss1"], dig["flat_g1"] = _sha(ft.step(x, y)), _sha(ft.flat_g)
        dig["scores_eval"] = _sha(ft.score(x, y))
        dig["loss2"] = _sha(ft.step(x, y))
    dig.update(flat_g=_sha(ft.flat_g), flat_p=_sha(ft.flat_p), scores=_sha(ft.scores))
    return trace, dig


def _reload_other_seed(proxy):
    from allrank_amd.engine import FusedTrainer
    trace, dig = [], {}
    with _recording(proxy, trace):
        ft = FusedTrainer(_model(**SMALL), "listNet", {}, 5, 70, use_graph=False, seed=1234)
        x, y, _, _ = _batch(SMALL_LENS, 70, 20, 3)
        dig["loss1"] = _sha(ft.step(x, y))
        sd = ft.state_dict()
        dig["state"] = _sha(torch.cat([t.reshape(-1) for n in sorted(sd["params"])
                                       for t in [sd["params"][n]] + [sd["optimizer"]["state"][n][k] for k in sorted(sd["optimizer"]["state"][n])]]))
        dig["meta"] = _sha_bytes(json.dumps(sd["meta"], sort_keys=True, default=repr).encode())
        ft.load_state_dict(dict(sd, seed=(sd["seed"] + 77) & 0xFFFFFFFF))
        dig["loaded"] = _sha(torch.cat([ft.flat_p, ft.flat_m, ft.flat_v, ft.step_count]))
        dig["loss2"] = _sha(ft.step(x, y))
    dig.update(flat_g=_sha(ft.flat_g), flat_p=_sha(ft.flat_p), scores=_sha(ft.scores))
    return trace, dig


def _scorer_input_norm_46(proxy):
    from allrank_amd.engine import FusedTrainer
    trace = []
    with _recording(proxy, trace):
        ft = FusedTrainer(_model(**dict(SMALL, F=46, input_norm=True)), "listNet", {}, 5, 70, use_graph=False, seed=1234)
        xt, yt, _, _ = _batch(SMALL_LENS, 70, 46, 3)
        ft.step(xt, yt)
        sc = ft.scorer(5, 90, use_graph=False)
        x, y, _, hl = _batch(SCORER_LENS, 90, 46, 4)
        raw = sc.run(x, y, lengths=hl)
        dig = _packed_digests(sc, raw)
    return trace, dig


def options_cases():
    """the fourth set: every A/B switch of the large-tile step off on its own, and the paths of construction, scoring and state I/O
    the first three sets do not reach; every trace begins at the constructor"""
    def large(model_kw=LARGE, **kw):
        return lambda p: _train(p, model_kw, "approxNDCGLoss", {}, LARGE_LENS, 128, construct=True, **kw)
    fc3 = dict(SMALL, sizes=[48, 40, 32], act="ReLU", fc_dropout=0.2)
    pe = dict(SMALL, pe=dict(strategy="fixed", max_indices=100))
    return {
        "large_weight_images_off": large(weight_images=False),
        "large_group_wgrad_off": large(group_wgrad=False),
        "large_ln_in_wgrad_off": large(ln_in_wgrad=False),
        "large_norm_head_off": large(_norm_head=False),
        "large_pad_input_off": large(pad_input=False),
        # both sublayer dropouts on: the dropout buffer is reused between the branches, so the layer's weight gradients run as two
        # groups of two
        "large_sublayer_dropout": large(dict(LARGE, dropout=0.1)),
        "fc_stack_three_relu_dropout": lambda p: _train(p, fc3, "listNet", {}, SMALL_LENS, 70, construct=True),
        "fixed_pe_grid": lambda p: _train(p, pe, "listNet", {}, SMALL_LENS, 70, use_idx=True, construct=True),
        "step_score_step": _step_score_step,
        "reload_other_seed": _reload_other_seed,
        "scorer_input_norm_46": _scorer_input_norm_46,
    }


# ------------------------------------------------------------------------------------------------------------------
# the fifth set: whole fit() calls
# ------------------------------------------------------------------------------------------------------------------
FIT_F, FIT_L, FIT_BS = 20, 20, 16                                            # 40 queries of 3..20 items: batches of 16, 16 and a short 8
_FIT_DATA = {}
_WALL_CLOCK_AND_PATHS = ("train_s", "val_s", "ckpt_s", "path")


def _fit_arrays(role):
    """(lengths, X, y) of one file: features on the 4-decimal grid of [0, 1) (the text holds them exactly), labels 0..4"""
    rng = np.random.default_rng({"train": 21, "vali": 22, "vali_long": 23}[role])
    if role == "train":
        lens = rng.integers(3, FIT_L + 1, 40)
    else:
        lens = rng.integers(3, FIT_L + 1, 24)
        lens[7] = FIT_L if role == "vali" else 27                 # "vali": the training step's slate length, so trainer.score() serves it
    n = int(lens.sum())
    X = (rng.integers(0, 10000, (n, FIT_F)) / 10000.0).astype(np.float32)
    w = rng.standard_normal(FIT_F)
    y = np.clip(np.round((X.astype(np.float64) - 0.5) @ w * 1.2 + 1.5), 0, 4).astype(np.float32)
    return lens, X, y


def _fit_data():
    """the libsvm files (written once per process into a temp dir), the resident sets read back from them, and the same slates as
    padded host tensors for a plain DataLoader"""
    import tempfile
    from allrank_amd import data as ED
    if not _FIT_DATA:
        root = tempfile.mkdtemp(prefix="call_trace_fit_")
        atexit.register(shutil.rmtree, root, ignore_errors=True)
        host = {}
        for role in ("train", "vali", "vali_long"):
            lens, X, y = _fit_arrays(role)
            d = os.path.join(root, "long" if role == "vali_long" else "same")
            os.makedirs(d, exist_ok=True)
            q = np.repeat(np.arange(len(lens)), lens)
            for path in [os.path.join(d, role.split("_")[0] + ".txt")] + ([os.path.join(root, "long", "train.txt")] if role == "train" else []):
                os.makedirs(os.path.dirname(path), exist_ok=True)
                with open(path, "w") as fh:
                    for i in range(len(y)):
                        fh.write("%d qid:%d %s\n" % (int(y[i]), 100 + q[i], " ".join("%d:%.4f" % (k + 1, X[i, k]) for k in range(FIT_F))))
            L = FIT_L if role == "train" else int(lens.max())
            xp, yp = np.zeros((len(lens), L, FIT_F), np.float32), np.full((len(lens), L), -1.0, np.float32)
            ip, o = np.full((len(lens), L), -1, np.int64), 0
            for b, k in enumerate(lens):
                xp[b, :k], yp[b, :k], ip[b, :k] = X[o:o + k], y[o:o + k], np.arange(k)
                o += k
            host[role] = (torch.tensor(xp), torch.tensor(yp), torch.tensor(ip))
        _FIT_DATA.update(host=host, same=ED.load_libsvm_dataset(os.path.join(root, "same"), FIT_L, "vali", device=DEV),
                         long=ED.load_libsvm_dataset(os.path.join(root, "long"), FIT_L, "vali", device=DEV))
    return _FIT_DATA


def _fit_loaders(kind, vali, nan):
    from torch.utils.data import DataLoader, TensorDataset
    from allrank_amd import data as ED
    d = _fit_data()
    if kind == "device":
        tr, va = d["long" if vali == "long" else "same"]
        return ED.DeviceLoader(tr, FIT_BS, shuffle=True, sampling="device"), ED.DeviceLoader(va, FIT_BS, shuffle=False)
    xt, yt, it = d["host"]["train"]
    if nan:
        xt = xt.clone()
        xt[5, 0, 3] = float("nan")
    return (DataLoader(TensorDataset(xt, yt, it), batch_size=FIT_BS, shuffle=False),
            DataLoader(TensorDataset(*d["host"]["vali_long" if vali == "long" else "vali"]), batch_size=FIT_BS, shuffle=False))


def _canon(v):
    """a value as JSON that keeps its type: tensors by digest, floats as float.hex, wall-clock entries and paths dropped"""
    if torch.is_tensor(v):
        return ["tensor", str(v.dtype), list(v.shape), _sha(v)]
    if isinstance(v, dict):
        return {str(k): _canon(x) for k, x in sorted(v.items(), key=lambda kv: str(kv[0])) if k not in _WALL_CLOCK_AND_PATHS}
    if isinstance(v, (list, tuple)):
        return [type(v).__name__, [_canon(x) for x in v]]
    if isinstance(v, (float, np.floating)):
        return [type(v).__name__, float(v).hex()]
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        return [type(v).__name__, str(int(v))]
    return [type(v).__name__, repr(v)]


def _digest(v):
    return _sha_bytes(json.dumps(_canon(v), sort_keys=True).encode())


@contextlib.contextmanager
def _score_sources(model, seen):
    """count, per validation score source, the batches it served: FusedScorer.run_resident, FusedScorer.run, FusedTrainer.score and
    the nn.Module forward with autograd off (a training forward of the autograd engine runs with it on)"""
    from allrank_amd import engine as EN
    saved = []

    def counted(cls, name, key):
        fn = getattr(cls, name)
        saved.append((cls, name, fn))

        def wrapper(*a, **kw):
            seen[key] = seen.get(key, 0) + 1
            return fn(*a, **kw)
        setattr(cls, name, wrapper)
    counted(EN.FusedScorer, "run_resident", "resident")
    counted(EN.FusedScorer, "run", "packed")
    counted(EN.FusedTrainer, "score", "trainer_score")
    hook = model.register_forward_hook(lambda *a: None if torch.is_grad_enabled() else seen.__setitem__("module", seen.get("module", 0) + 1))
    try:
        yield
    finally:
        hook.remove()
        for cls, name, fn in saved:
            setattr(cls, name, fn)


def _fit_case(loss=("listNet", {}), loaders="device", vali="same", model_kw=None, opt=("Adam", dict(lr=2e-3)), sched=None, epochs=3,
              patience=10, nan=False, resume_to=None, **fit_kw):
    """one fit() job as a case: returns run(proxy) -> (trace, digests, notes).  ``resume_to``: the job is run for ``epochs`` epochs,
    then built afresh under other seeds and continued with resume="auto" up to ``resume_to`` -- both calls in one trace"""
    def build(seeds):
        from allrank_amd import losses as E
        model = _model(**dict(dict(F=FIT_F, sizes=[32], N=1, d_ff=64, h=4, dropout=0.1), **(model_kw or {})))
        torch.manual_seed(seeds[0]), np.random.seed(seeds[1])
        o = getattr(torch.optim, opt[0])(model.parameters(), **opt[1])
        s = None if sched is None else getattr(torch.optim.lr_scheduler, sched[0])(o, **sched[1])
        return model, functools.partial(getattr(E, loss[0]), **loss[1]), o, s

    def call(proxy, trace, out_dir, seeds, n_epochs, notes, **kw):
        import types
        from allrank_amd import fit as EF
        model, loss_func, o, s = build(seeds)
        train_dl, valid_dl = _fit_loaders(loaders, vali, nan)
        cfg = types.SimpleNamespace(metrics={"ndcg": [5], "mrr": [10]}, val_metric="ndcg_5")
        res, seen = None, notes.setdefault("sources", {})
        with _recording(proxy, trace), _score_sources(model, seen):
            try:
                res = EF.fit(epochs=n_epochs, model=model, loss_func=loss_func, optimizer=o, scheduler=s, train_dl=train_dl, valid_dl=valid_dl,
                             config=cfg, gradient_clipping_norm=None, early_stopping_patience=patience, device=torch.device(DEV),
                             output_dir=out_dir, tensorboard_output_path=None, **dict(fit_kw, **kw))
            except FloatingPointError as e:
                notes["error"] = str(e)
        torch.cuda.synchronize()
        return res, dict(EF.last_run), o

    def run(proxy):
        import tempfile
        with tempfile.TemporaryDirectory(prefix="call_trace_fit_out_") as out_dir:
            return job(proxy, out_dir)

    def job(proxy, out_dir):
        trace, dig, notes = [], {}, {}
        parts = [("", (42, 43), epochs, {})] if resume_to is None else [("first_", (42, 43), epochs, {}), ("", (52, 53), resume_to, dict(resume="auto"))]
        for tag, seeds, n_epochs, kw in parts:
            res, last, o = call(proxy, trace, out_dir, seeds, n_epochs, notes, **kw)
            notes.update(engine=last.get("engine"), fcstep=bool(last.get("fcstep")), compact=last.get("compact"), val_scorer=last.get("val_scorer"),
                         val_scorer_reason=last.get("val_scorer_reason"), val_eval=last.get("val_eval"),
                         compact_graph=last.get("compact_graph") is not None, epochs=None if res is None else int(res["epochs"]))
            dig[tag + "last_run"] = _digest(last)
            dig[tag + "val_loss"] = _digest([e["val_loss"] for e in last.get("epoch_log", [])])
            dig[tag + "lr"] = _digest(o.param_groups[0]["lr"])
            if "error" in notes:
                dig[tag + "error"] = _sha_bytes(notes["error"].encode())
                continue
            dig[tag + "result"] = _digest(res)
            dig[tag + "model_pkl"] = _digest(torch.load(os.path.join(out_dir, "model.pkl"), map_location="cpu"))
            if "checkpoint_every" in fit_kw:
                from allrank_amd import checkpoint as CK
                ck = CK.load(os.path.join(out_dir, "checkpoint.pt"))
                dig[tag + "ckpt_trainer"] = _digest(ck["trainer"])
                dig[tag + "ckpt_rest"] = _digest({k: v for k, v in ck.items() if k not in ("trainer", "rng")})
        return trace, dig, notes
    return run


def fit_cases():
    """the fifth set: whole ``fit()`` calls over a small libsvm set -- both engines, the four validation score sources, the ragged
    evaluation, schedulers, early stopping, the finiteness check and checkpoint / resume"""
    step_lr = ("StepLR", dict(step_size=1, gamma=0.5))
    ordinal = dict(loss=("ordinal", {"n": 3}), model_kw=dict(d_output=3, out_act="Sigmoid"))
    ckpt = dict(sched=step_lr, epochs=2, resume_to=4, checkpoint_every=1)
    return {
        "fit_fused_grid_trainer_score": _fit_case(compact=False, val_scorer="module"),
        "fit_fused_grid_module_val": _fit_case(compact=False, val_scorer="module", vali="long"),
        "fit_fused_compact": _fit_case(compact=True),
        "fit_fused_compact_graph_packed_val": _fit_case(compact="graph", val_scorer="packed"),
        "fit_fused_host_loader_ragged_val": _fit_case(loaders="host", val_scorer="ragged", vali="long"),
        "fit_autograd_step_lr": _fit_case(use_fused=False, sched=step_lr),
        "fit_autograd_reference_metrics_plateau": _fit_case(use_fused=False, train_metrics="reference",
                                                            sched=("ReduceLROnPlateau", dict(mode="max", factor=0.5, patience=0))),
        "fit_fused_step_lr_early_stop": _fit_case(opt=("Adam", dict(lr=0.05)), sched=("StepLR", dict(step_size=2, gamma=0.5)), epochs=8,
                                                  patience=0),
        "fit_fc_listnet_step": _fit_case(model_kw=dict(N=0), compact=True),
        "fit_stochastic_neural_ndcg_packed_val": _fit_case(loss=("neuralNDCG", dict(stochastic=True, n_samples=4)), val_scorer="packed"),
        "fit_ordinal_fused": _fit_case(**ordinal),
        "fit_ordinal_autograd": _fit_case(use_fused=False, **ordinal),
        "fit_check_finite_healthy": _fit_case(check_finite=True),
        "fit_check_finite_nan_fused": _fit_case(loaders="host", nan=True, check_finite=True),
        "fit_check_finite_nan_autograd": _fit_case(loaders="host", nan=True, check_finite=True, use_fused=False),
        "fit_checkpoint_resume_fused": _fit_case(**ckpt),
        "fit_checkpoint_resume_autograd": _fit_case(use_fused=False, **ckpt),
    }


SETS = {"calls": (FIXTURE, cases), "rows": (ROWS_FIXTURE, rows_cases), "step": (STEP_FIXTURE, step_cases),
        "options": (OPTIONS_FIXTURE, options_cases), "fit": (FIT_FIXTURE, fit_cases)}


def run_case(proxy, name):
    """(trace, digests, notes) of one case; ``notes`` ({} outside the fit set): plain facts about the run, held like the digests"""
    got = {n: f for _, make in SETS.values() for n, f in make().items()}[name](proxy)
    torch.cuda.synchronize()
    return got if len(got) == 3 else got + ({},)


def record(names):
    rec = {}
    with proxied() as proxy:
        for name in names:
            (t1, d1, n1), (t2, d2, n2) = run_case(proxy, name), run_case(proxy, name)
            assert t1 == t2, "%s: the two runs made different calls" % name
            assert t1, "%s: no call recorded" % name
            assert n1 == n2, "%s: the two runs differ in %s" % (name, sorted(k for k in n1 if n1[k] != n2.get(k)))
            rec[name] = dict(trace=t1, digests={k: v for k, v in d1.items() if d2[k] == v},
                             unstable=sorted(k for k, v in d1.items() if d2[k] != v), notes=n1)
            print("%-36s %4d calls, %d digests, unstable: %s %s" % (name, len(t1), len(rec[name]["digests"]), rec[name]["unstable"],
                                                                    json.dumps(n1, sort_keys=True) if n1 else ""), flush=True)
    return rec


def expand(rec):
    """a loaded fixture with every trace as the list of calls: the fit set stores each distinct call once ("calls") and a trace as
    indices into that table -- the steps of a fit() repeat their calls, and the file stays small"""
    table = rec.get("calls")
    if table is not None:
        for c in rec["cases"].values():
            c["trace"] = [table[i] for i in c["trace"]]
    return rec


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="calls", choices=sorted(SETS), help="which case set to record")
    ap.add_argument("--out", default=None, help="(default: the set's own file)")
    ap.add_argument("--commit", default=None, help="the checked-out commit (default: asked of git)")
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"]).decode().strip()
    path, names = SETS[args.set]
    out = args.out or path
    rec = record(names())
    table = {}
    with open(out, "w") as fh:                           # one call per line: a changed argument is a one-line diff
        fh.write('{"commit": %s,\n "cases": {' % json.dumps(commit))
        for i, (name, c) in enumerate(rec.items()):
            head = '%s\n  %s: {"digests": %s,\n   "unstable": %s,\n' % ("," if i else "", json.dumps(name), json.dumps(c["digests"], sort_keys=True),
                                                                       json.dumps(c["unstable"]))
            if args.set == "fit":                        # (see ``expand``)
                idx = [table.setdefault(json.dumps(call), len(table)) for call in c["trace"]]
                fh.write('%s   "notes": %s,\n   "trace": %s}' % (head, json.dumps(c["notes"], sort_keys=True), json.dumps(idx, separators=(",", ":"))))
            else:
                fh.write('%s   "trace": [\n    %s\n   ]}' % (head, ",\n    ".join(json.dumps(call) for call in c["trace"])))
        fh.write("\n }")
        if table:
            fh.write(',\n "calls": [\n  %s\n ]' % ",\n  ".join(table))
        fh.write("\n}\n")
    print("wrote %s: %d cases, %d calls" % (out, len(rec), sum(len(c["trace"]) for c in rec.values())))


if __name__ == "__main__":
    main()
