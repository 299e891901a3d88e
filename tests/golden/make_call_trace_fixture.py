"""Record which libltrx calls the package makes, and what they compute, over a set of small cases (needs the MI355X).

    python tests/golden/make_call_trace_fixture.py [--set calls|rows|step|options] [--out FILE] [--commit HASH]

Four case sets, one file each, each run ONCE at the commit named in its file ("commit"):
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
import contextlib
import ctypes
import hashlib
import json
import os
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


SETS = {"calls": (FIXTURE, cases), "rows": (ROWS_FIXTURE, rows_cases), "step": (STEP_FIXTURE, step_cases),
        "options": (OPTIONS_FIXTURE, options_cases)}


def run_case(proxy, name):
    trace, dig = {n: f for _, make in SETS.values() for n, f in make().items()}[name](proxy)
    torch.cuda.synchronize()
    return trace, dig


def record(names):
    rec = {}
    with proxied() as proxy:
        for name in names:
            (t1, d1), (t2, d2) = run_case(proxy, name), run_case(proxy, name)
            assert t1 == t2, "%s: the two runs made different calls" % name
            assert t1, "%s: no call recorded" % name
            rec[name] = dict(trace=t1, digests={k: v for k, v in d1.items() if d2[k] == v},
                             unstable=sorted(k for k, v in d1.items() if d2[k] != v))
            print("%-36s %4d calls, %d digests, unstable: %s" % (name, len(t1), len(rec[name]["digests"]), rec[name]["unstable"]), flush=True)
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
    with open(out, "w") as fh:                           # one call per line: a changed argument is a one-line diff
        fh.write('{"commit": %s,\n "cases": {' % json.dumps(commit))
        for i, (name, c) in enumerate(rec.items()):
            fh.write('%s\n  %s: {"digests": %s,\n   "unstable": %s,\n   "trace": [\n    %s\n   ]}'
                     % ("," if i else "", json.dumps(name), json.dumps(c["digests"], sort_keys=True), json.dumps(c["unstable"]),
                        ",\n    ".join(json.dumps(call) for call in c["trace"])))
        fh.write("\n }\n}\n")
    print("wrote %s: %d cases, %d calls" % (out, len(rec), sum(len(c["trace"]) for c in rec.values())))


if __name__ == "__main__":
    main()
