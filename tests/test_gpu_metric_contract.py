"""The contract of the metric kernels (allrank_amd/csrc/ltrx_ndcg.hip: ltrx_ndcg_at, ltrx_ndcg_at_gains, ltrx_ndcg_at_cu;
allrank_amd/csrc/ltrx_pointpair.hip: ltrx_mrr_at, ltrx_mrr_at_cu; padded and cu_seqlens layouts, 256 and 1024 threads, below and above the
default dynamic LDS allowance), -m gpu.

One call through the C ABI per comparison and one assertion for EVERY entry of every output: |kernel - fp64 reference| <= bar for every
ndcg and dcg entry; the filler entries, order_out over the whole slate (padded tail included), MRR's per-slate (best_val, best_idx) at the
head of its workspace and the whole MRR output (against the fp32 transcription) bit for bit.  The references, the derivation of the bars,
the defect models and the case table are in tests/metric_ref.py; tests/test_metric_ref_cpu.py is the evidence that the bars bite.

Around every window the buffers hold sentinels (NaN around outputs, 3e37 around inputs, a fill value around the integer arrays, 0xA5 behind
an MRR workspace of exactly ltrx_mrr_workspace_bytes, NaN inside it before the call; NDCG's workspace is 0 bytes: NULL is passed) that must
survive; inputs must be unchanged; a second identical call gives the same bits; calls with dcg_out = NULL and order_out = NULL give the
same ndcg bits; a slate that slate_order never names keeps what its outputs held.  At every length of EXPECTED_ARMS the thread count and
the opt-in are the table's literals.  The worst error / bar of every (kernel, arm, case, output) is logged as parity_metric_contract.json."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import metric_ref as R
from tests.test_gpu_gemm_contract import EINVAL, EUNSUPPORTED, GARBAGE, Win
from tests.test_gpu_parity import DEV, _log
from tests.test_gpu_step_kernels import Raw

pytestmark = pytest.mark.gpu

F = np.float32
TAIL = 4096
ROWS = {}
T0 = time.time()
ORDER_FILL = -7
INT_FILL = 0x5A5A5A5A


def _libs():
    from allrank_amd import _lib as LB
    return LB, LB.lib()


def _run(what, fn):
    """a library call; after a device error nothing more is launched"""
    LB, _ = _libs()
    try:
        LB.check(fn(), what)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "hip" in str(e).lower():
            pytest.exit("%s: %s -- nothing more is launched on a device that reported an error" % (what, e), returncode=3)
        raise


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _in(data):
    data = np.atleast_2d(np.asarray(data, F))
    return Win(data.shape, data.shape[1], 4, GARBAGE, data)


def _out(rows, cols):
    return Win((rows, cols), cols, 4, np.nan)


def _ats(ats):
    return (ctypes.c_int * len(ats))(*[int(a) for a in ats])


class Problem(object):
    """one case on the device: its input windows and one call of its entry point"""

    def __init__(self, c):
        self.c = c
        self.bt, gains = R.inputs(c)
        bt = self.bt
        self.shape = (1, bt.s.shape[0]) if bt.ragged else bt.s.shape
        self.ins = dict(s=_in(bt.s.reshape(self.shape)), y=_in(bt.y.reshape(self.shape)))
        if gains is not None:
            self.ins["gains"] = _in(gains)
        if bt.ragged:
            self.ins["cu"] = Raw(bt.cu, np.int32, INT_FILL)
            if bt.order is not None:
                self.ins["order"] = Raw(bt.order, np.int32, INT_FILL)

    def call(self, extras=True):
        """{output: array} of one call; extras False passes NULL for dcg_out and order_out"""
        _, lib = _libs()
        c, bt, ins = self.c, self.bt, self.ins
        B, L, n_ats = bt.B, bt.L, len(c.ats)
        what = "%s (extras %s)" % (c.name, extras)
        cu = ins["cu"].ptr if bt.ragged else None
        so = ins["order"].ptr if "order" in ins else None
        res = _out(B, n_ats)
        ats = _ats(c.ats)
        if R.is_mrr(c):
            nws = lib.ltrx_mrr_workspace_bytes(B, L, n_ats)
            assert nws == R.mrr_workspace_bytes(B), "%s: the library sizes its workspace as %d bytes, the restated rule as %d" % (c.name, nws, R.mrr_workspace_bytes(B))
            ws = torch.full((nws + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
            ws[nws:] = 0xA5
            wsp = ctypes.c_void_p(ws.data_ptr())
            if bt.ragged:
                fn = lambda: lib.ltrx_mrr_at_cu(ins["s"].ptr, ins["y"].ptr, cu, so, B, L, ats, n_ats, res.ptr, wsp, None)   # noqa: E731
            else:
                fn = lambda: lib.ltrx_mrr_at(ins["s"].ptr, ins["y"].ptr, B, L, ats, n_ats, float(R.PAD), res.ptr, wsp, None)   # noqa: E731
            _run(what, fn)
            assert bool((ws[nws:] == 0xA5).all()), "%s: wrote behind its %d-byte workspace" % (what, nws)
            head = ws[:8 * B].cpu().numpy()
            return dict(mrr=res.fetch(what + " mrr"), best_val=head[:4 * B].view(F).copy(), best_idx=head[4 * B:].view(np.int32).copy())
        assert lib.ltrx_ndcg_workspace_bytes(B, L) == 0
        dcg = _out(B, n_ats) if extras else None
        order = Raw(np.full(bt.s.size, ORDER_FILL), np.int64, ORDER_FILL) if extras else None
        P = lambda x: x.ptr if x is not None else None      # noqa: E731
        fill = float(R.FILLER)
        if c.entry == "ltrx_ndcg_at":
            fn = lambda: lib.ltrx_ndcg_at(ins["s"].ptr, ins["y"].ptr, B, L, ats, n_ats, float(R.PAD), fill, res.ptr, P(dcg), P(order), None, None)   # noqa: E731
        elif c.entry == "ltrx_ndcg_at_gains":
            fn = lambda: lib.ltrx_ndcg_at_gains(ins["s"].ptr, ins["y"].ptr, ins["gains"].ptr, B, L, ats, n_ats, float(R.PAD), fill, res.ptr, P(dcg),   # noqa: E731
                                                P(order), None, None)
        else:
            fn = lambda: lib.ltrx_ndcg_at_cu(ins["s"].ptr, ins["y"].ptr, cu, so, B, L, ats, n_ats, fill, res.ptr, P(dcg), P(order), None, None)   # noqa: E731
        _run(what, fn)
        out = dict(ndcg=res.fetch(what + " ndcg"))
        if extras:
            out["dcg"] = dcg.fetch(what + " dcg")
            out["order"] = order.fetch(what + " order_out").reshape(bt.s.shape)
        return out

    def inputs_unchanged(self):
        for name, wnd in self.ins.items():
            wnd.unchanged("%s %s" % (self.c.name, name))


def _kernel(c):
    return ("ltrx_mrr_slate_kernel<%s>" if R.is_mrr(c) else "ltrx_ndcg_kernel<%s>") % ("true" if c.entry.endswith("_cu") else "false")


def _arm(c):
    return "%d threads%s" % (R.threads(c.entry, c.L), ", LDS opt-in" if R.opts_in(c.entry, c.L) else "")


def _contract(c):
    ref = R.reference(c)
    arm = (R.threads(c.entry, c.L), R.opts_in(c.entry, c.L))
    assert arm == R.EXPECTED_ARMS.get((c.entry, c.L), arm), "%s: the restated rule gives %s, the table of switch lengths %s" % (
        c.name, arm, R.EXPECTED_ARMS.get((c.entry, c.L)))
    pr = Problem(c)
    got = pr.call()
    for k, (g, r, bar) in R.checks(c, got, ref).items():
        ratio = R.worst(g, r, bar)
        key = (_kernel(c), _arm(c), c.name, k)
        ROWS[key] = max(ROWS.get(key, 0.0), ratio)
        print("%s [%s]: %s worst error / bar %.4g" % (c.name, _arm(c), k, ratio))
        assert ratio <= 1.0, "%s [%s]: %s is outside its bar at %d of %d entries, worst error / bar %.4g" % (
            c.name, _arm(c), k, int(R.over(g, r, bar).sum()), np.asarray(g).size, ratio)
    assert R.exact_ok(c, got, ref), "%s: an exact output (order_out, a filler entry, best_val / best_idx, the MRR bits) differs" % c.name
    if not R.is_mrr(c):
        skip = ~ref["visited"]
        rows = np.repeat(skip, np.diff(pr.bt.cu)) if pr.bt.ragged else np.repeat(skip, pr.bt.L).reshape(pr.bt.s.shape)
        assert np.isnan(got["ndcg"][skip]).all() and np.isnan(got["dcg"][skip]).all() and (got["order"][rows] == ORDER_FILL).all(), (
            "%s: a slate that slate_order does not name was written" % c.name)
        empty = np.array([len(s) == 0 for s, _, _ in pr.bt.slates()]) & ref["visited"]
        assert not got["dcg"][empty].any(), "%s: the DCG of an empty slate is not 0" % c.name
    twice = pr.call()
    for k in got:
        a, b = np.asarray(got[k]), np.asarray(twice[k])
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype.kind == "f" else np.array_equal(a, b), "%s: a second call gives other bits in %s" % (c.name, k)
    if not R.is_mrr(c):
        other = pr.call(extras=False)
        assert np.array_equal(_bits(other["ndcg"]), _bits(got["ndcg"])), "%s: dcg_out = NULL and order_out = NULL change the ndcg bits" % c.name
    pr.inputs_unchanged()


def _log_rows():
    _log("metric_contract", dict(seconds_since_import=time.time() - T0,
                                 rows=[dict(kernel=k[0], arm=k[1], case=k[2], output=k[3], worst_error_over_bar=v) for k, v in sorted(ROWS.items())]))


GROUPS = sorted({(c.entry, c.L) for c in R.CASES})


@pytest.mark.parametrize("entry,L", [pytest.param(*g, id="%s L %d %d threads%s" % (g + (R.threads(*g), " opt-in" if R.opts_in(*g) else ""))) for g in GROUPS])
def test_metric_meets_the_entrywise_contract(entry, L):
    t0 = time.time()
    for c in [c for c in R.CASES if (c.entry, c.L) == (entry, L)]:
        _contract(c)
    _log_rows()
    print("%s L %d: %.2f s" % (entry, L, time.time() - t0))


def test_refusals_return_without_writing():
    _, lib = _libs()
    B, L = 3, 8
    rng = np.random.default_rng(9)
    s, y, gains = _in(rng.standard_normal((B, L))), _in(rng.integers(0, 5, (B, L))), _in(rng.uniform(0, 1, (B, L)))
    cu = Raw([0, 8, 16, 24], np.int32, INT_FILL)
    outs = dict(ndcg=_out(B, 3), dcg=_out(B, 3), mrr=_out(B, 3))
    order = Raw(np.full(B * L, ORDER_FILL), np.int64, ORDER_FILL)
    ws = torch.zeros(1 << 12, dtype=torch.uint8, device=DEV)
    D = dict(s=s.ptr, y=y.ptr, gains=gains.ptr, cu=cu.ptr, B=B, L=L, ats=(1, 5, 9), n_ats=None, ndcg=outs["ndcg"].ptr, dcg=outs["dcg"].ptr, order=order.ptr,
             mrr=outs["mrr"].ptr, ws=ctypes.c_void_p(ws.data_ptr()))

    def args(kw):
        a = dict(D, **kw)
        a["n"] = len(a["ats"]) if a["n_ats"] is None else a["n_ats"]
        a["arr"] = None if a["ats"] is None else _ats(a["ats"])
        return a

    def ndcg(**kw):
        a = args(kw)
        return lib.ltrx_ndcg_at(a["s"], a["y"], a["B"], a["L"], a["arr"], a["n"], -1.0, 1.0, a["ndcg"], a["dcg"], a["order"], None, None)

    def ndcg_gains(**kw):
        a = args(kw)
        return lib.ltrx_ndcg_at_gains(a["s"], a["y"], a["gains"], a["B"], a["L"], a["arr"], a["n"], -1.0, 1.0, a["ndcg"], a["dcg"], a["order"], None, None)

    def ndcg_cu(**kw):
        a = args(kw)
        return lib.ltrx_ndcg_at_cu(a["s"], a["y"], a["cu"], None, a["B"], a["L"], a["arr"], a["n"], 1.0, a["ndcg"], a["dcg"], a["order"], None, None)

    def mrr(**kw):
        a = args(kw)
        return lib.ltrx_mrr_at(a["s"], a["y"], a["B"], a["L"], a["arr"], a["n"], -1.0, a["mrr"], a["ws"], None)

    def mrr_cu(**kw):
        a = args(kw)
        return lib.ltrx_mrr_at_cu(a["s"], a["y"], a["cu"], None, a["B"], a["L"], a["arr"], a["n"], a["mrr"], a["ws"], None)

    common = (dict(s=None), dict(y=None), dict(ats=None, n_ats=3), dict(B=0), dict(B=-2), dict(L=0), dict(L=-1), dict(n_ats=0))
    for fn in (ndcg, ndcg_gains, ndcg_cu, mrr, mrr_cu):
        for kw in common:
            assert fn(**kw) == EINVAL, (fn.__name__, sorted(kw))
        assert fn(L=R.MAX_METRIC_L + 1) == EUNSUPPORTED, fn.__name__
        assert fn(ats=tuple(range(1, R.MAX_ATS + 2))) == EUNSUPPORTED, fn.__name__
    for fn in (ndcg, ndcg_gains, ndcg_cu):
        assert fn(ndcg=None) == EINVAL, fn.__name__
        for ats in ((0, 5, 9), (1, 5, -3)):
            assert fn(ats=ats) == EINVAL, (fn.__name__, ats)
    for fn in (mrr, mrr_cu):
        assert fn(mrr=None) == EINVAL and fn(ws=None) == EINVAL, fn.__name__
    assert ndcg_gains(gains=None) == EINVAL and ndcg_cu(cu=None) == EINVAL and mrr_cu(cu=None) == EINVAL
    torch.cuda.synchronize()
    for name, wnd in outs.items():
        wnd.unchanged("a refused call wrote " + name)
    order.unchanged("a refused call wrote order_out")
    for wnd in (s, y, gains, cu):
        wnd.unchanged("a refused call wrote an input")
    assert not bool(ws.any()), "a refused call wrote its workspace"
    assert lib.ltrx_mrr_workspace_bytes(0, 0, 0) == R.mrr_workspace_bytes(0) and lib.ltrx_mrr_workspace_bytes(-3, 5, 1) == 64


def test_metric_wrappers_equal_the_abi_calls_bit_for_bit():
    """metrics.ndcg / dcg / mrr and their allrank_amd.ragged forms are the same ABI calls: the same bits on one case per entry, so the
    contract carries over to the public surface (the only place the wrappers appear in this file)"""
    from allrank_amd import metrics as EM, ragged as RG
    t = lambda a: torch.tensor(np.asarray(a), device=DEV)      # noqa: E731
    pick = {}
    for c in R.CASES:
        if c.L == 257 and len(c.ats) in (3, 4) and c.order in (None, "perm"):
            pick[(c.entry, c.order)] = c
    for (entry, order), c in sorted(pick.items(), key=repr):
        bt, gains = R.inputs(c)
        got = Problem(c).call()
        s, y, ats = t(bt.s), t(bt.y), list(c.ats)
        if entry == "ltrx_ndcg_at":
            nd, od = EM.ndcg(s, y, ats=ats, filler_value=float(R.FILLER), return_order=True)
            out = dict(ndcg=nd, order=od, dcg=EM.dcg(s, y, ats=ats))
        elif entry == "ltrx_ndcg_at_gains":
            fn = lambda lab: lab + 1      # noqa: E731
            out = dict(ndcg=EM.ndcg(s, y, ats=ats, gain_function=fn, filler_value=float(R.FILLER)), dcg=EM.dcg(s, y, ats=ats, gain_function=fn))
        elif entry == "ltrx_mrr_at":
            out = dict(mrr=EM.mrr(s, y, ats=ats))
        else:
            kw = dict(cu_seqlens=t(bt.cu), max_len=c.L, slate_order=None if bt.order is None else t(bt.order), ats=ats)
            if entry == "ltrx_mrr_at_cu":
                out = dict(mrr=RG.mrr(s, y, **kw))
            else:
                nd, od = RG.ndcg(s, y, filler_value=float(R.FILLER), return_order=True, **kw)
                out = dict(ndcg=nd, order=od, dcg=RG.dcg(s, y, **kw))
        for k, v in out.items():
            v, g = v.cpu().numpy(), np.asarray(got[k])
            assert np.array_equal(v, g.reshape(v.shape)) if v.dtype.kind != "f" else np.array_equal(_bits(v), _bits(g).reshape(v.shape)), (c.name, k)
    assert {e for e, _ in pick} == set(R.NDCG_ENTRIES) | set(R.MRR_ENTRIES)
