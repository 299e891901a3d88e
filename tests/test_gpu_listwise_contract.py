"""The contract of the four listwise loss kernels (allrank_amd/csrc/ltrx_listnet.hip, ltrx_listmle.hip, ltrx_approxndcg.hip,
ltrx_lambdaloss.hip: listNet, listMLE, approxNDCG and lambdaLoss in all 8 schemes; padded and cu_seqlens layouts; the LDS arm, the LDS
arm that opts in to more than the default dynamic allowance, and the workspace (GWS) arm), -m gpu.

One call through the C ABI per comparison -- ltrx_listnet_fwd_bwd[_cu], ltrx_listmle_fwd_bwd, ltrx_approxndcg_fwd_bwd[_cu],
ltrx_lambdaloss_fwd_bwd[_cu] -- and one assertion for EVERY entry of every output: |kernel - fp64 reference| <= bar for every gradient
entry, every per-slate value and the loss; padded entries exactly 0; lambdaLoss's pair count and both order_out arrays exact.  The
references, the derivation of the entrywise bars, the branch guard, the defect models and the case table are in tests/listwise_ref.py;
tests/test_listwise_ref_cpu.py is the evidence that the bars bite (an fp32 transcription in the kernels' operation order is inside them
on every case, every defect model outside) and lists the defects that the max-norm bar of test_gpu_parity.py / test_gpu_score_scale.py /
test_gpu_ragged.py (tests.cases.grad_close) lets through.

Around every window the buffers hold sentinels (NaN around outputs, 3e37 around inputs, 0xA5 behind a workspace of exactly
ltrx_*_workspace_bytes(B, L), NaN inside it before the call) that must survive; inputs must be unchanged; a second identical call gives
the same bits; calls with grad_out = NULL and per_slate_out = NULL (lambdaLoss: pair_count_out and order_out) give the same loss bits.
For every case the library's workspace size is the one the restated array count and budget give (tests/listwise_ref.py: in_lds, held to
the source by source_constants) -- it holds the work arrays exactly when the workspace arm is taken --, and at every threshold length
the arm is the literal of EXPECTED_ARMS, so a moved threshold moves the cases or fails.  lambdaLoss returns no per-slate values through
the ABI: they are read from the head of its workspace (per_loss [B], per_cnt [B]).

test_gpu_score_scale.py::test_fused_loss_equals_the_plugin_call_at_score_scale ties FusedLoss and the autograd plugin bit for bit to these
ABI calls, so the contract carries over to both.  The worst error / bar of every (kernel, arm, case, output) is logged as
parity_listwise_contract.json."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import listwise_ref as R
from tests.test_gpu_gemm_contract import EINVAL, EUNSUPPORTED, GARBAGE, Win
from tests.test_gpu_parity import DEV, _log
from tests.test_gpu_step_kernels import Raw

pytestmark = pytest.mark.gpu

F = np.float32
TAIL = 4096
ROWS = {}
T0 = time.time()
ORDER_FILL = -7


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


def _workspace(nbytes):
    ws = torch.full((nbytes + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)             # NaN inside: an entry read before it is written shows
    ws[nbytes:] = 0xA5
    assert ws.data_ptr() % 16 == 0
    return ws


class Problem(object):
    """one case on the device: its input windows and one call of its entry point"""

    def __init__(self, c):
        self.c, self.bt = c, R.inputs(c)
        bt = self.bt
        self.shape = (1, bt.s.shape[0]) if bt.ragged else bt.s.shape
        self.s, self.y = _in(bt.s.reshape(self.shape)), _in(bt.y.reshape(self.shape))
        self.ins = dict(s=self.s, y=self.y)
        if bt.ragged:
            self.ins["cu"] = Raw(bt.cu, np.int32, 0x5A5A5A5A)
            if bt.order is not None:
                self.ins["order"] = Raw(bt.order, np.int32, 0x5A5A5A5A)
        if c.loss == "listmle":
            self.ins["perm"] = Raw(R.perm_of(c), np.int64, -1)
        if c.loss == "lambdaloss" and c.par.ext is not None:
            self.ins["ext"] = _in([[c.par.ext]])

    def call(self, grad=True, extras=True):
        """{output: array} of one call; grad / extras False pass NULL for the gradient / for per_slate_out, pair_count_out and order_out"""
        _, lib = _libs()
        c, bt = self.c, self.bt
        B, L, bd = bt.B, bt.L, R.batch_divisor(c, bt)
        cu = self.ins["cu"].ptr if bt.ragged else None
        so = self.ins["order"].ptr if "order" in self.ins else None
        what = "%s (grad %s, extras %s)" % (c.name, grad, extras)
        nws = getattr(lib, "ltrx_%s_workspace_bytes" % c.loss)(B, L)
        assert nws == R.workspace_bytes(c.loss, B, L), "%s: the library sizes its workspace as %d bytes, the restated rule as %d" % (
            c.name, nws, R.workspace_bytes(c.loss, B, L))
        ws = _workspace(nws)
        wsp = ctypes.c_void_p(ws.data_ptr())
        loss, g = _out(1, 1), (_out(*self.shape) if grad else None)
        per = _out(1, B) if extras and c.loss != "lambdaloss" else None
        P = lambda x: x.ptr if x is not None else None      # noqa: E731
        order = cnt = None
        if c.loss == "listnet":
            if bt.ragged:
                fn = lambda: lib.ltrx_listnet_fwd_bwd_cu(self.s.ptr, self.y.ptr, cu, so, B, L, R.EPS, bd, loss.ptr, P(per), P(g), wsp, None)   # noqa: E731
            else:
                fn = lambda: lib.ltrx_listnet_fwd_bwd(self.s.ptr, self.y.ptr, B, L, R.EPS, float(R.PAD), bd, loss.ptr, P(per), P(g), wsp, None)   # noqa: E731
        elif c.loss == "listmle":
            order = Raw(np.full(B * L, ORDER_FILL), np.int64, ORDER_FILL) if extras else None
            fn = lambda: lib.ltrx_listmle_fwd_bwd(self.s.ptr, self.y.ptr, self.ins["perm"].ptr, B, L, R.EPS, float(R.PAD), bd, loss.ptr, P(per), P(g),   # noqa: E731
                                                  P(order), wsp, None)
        elif c.loss == "approxndcg":
            if bt.ragged:
                fn = lambda: lib.ltrx_approxndcg_fwd_bwd_cu(self.s.ptr, self.y.ptr, cu, so, B, L, R.EPS, c.par, bd, loss.ptr, P(per), P(g), wsp, None)   # noqa: E731
            else:
                fn = lambda: lib.ltrx_approxndcg_fwd_bwd(self.s.ptr, self.y.ptr, B, L, R.EPS, float(R.PAD), c.par, bd, loss.ptr, P(per), P(g), wsp, None)   # noqa: E731
        else:
            p = c.par
            order = Raw(np.full(bt.s.size, ORDER_FILL), np.int64, ORDER_FILL) if extras else None
            cnt = _out(1, 1) if extras else None
            ext = self.ins["ext"].ptr if p.ext is not None else None
            tail = (p.scheme, p.k, p.sigma, p.mu, int(p.mean), int(p.natural), ext, loss.ptr, P(cnt), P(g), P(order), wsp, None)
            if bt.ragged:
                fn = lambda: lib.ltrx_lambdaloss_fwd_bwd_cu(self.s.ptr, self.y.ptr, cu, so, B, L, R.EPS, *tail)   # noqa: E731
            else:
                fn = lambda: lib.ltrx_lambdaloss_fwd_bwd(self.s.ptr, self.y.ptr, B, L, R.EPS, float(R.PAD), *tail)   # noqa: E731
        _run(what, fn)
        assert bool((ws[nws:] == 0xA5).all()), "%s: wrote behind its %d-byte workspace" % (what, nws)
        out = dict(loss=loss.fetch(what + " loss")[0, 0])
        if g is not None:
            out["grad"] = g.fetch(what + " grad").reshape(bt.s.shape)
        if per is not None:
            out["per"] = per.fetch(what + " per-slate")[0]
        if c.loss == "lambdaloss":
            head = ws[:8 * B].view(torch.float32).cpu().numpy()
            out["per"], out["per_count"] = head[:B].copy(), head[B:].copy()
        if order is not None:
            out["order"] = order.fetch(what + " order_out").reshape(bt.s.shape)
        if cnt is not None:
            out["count"] = float(cnt.fetch(what + " pair count")[0, 0])
        return out

    def inputs_unchanged(self):
        for name, wnd in self.ins.items():
            wnd.unchanged("%s %s" % (self.c.name, name))


def _kernel(c):
    return "ltrx_%s_kernel<%s%s>" % (c.loss, "true" if c.arm == "GWS" else "false", "" if c.loss == "listmle" else (", true" if c.layout == "ragged" else ", false"))


def _contract(c):
    ref = R.reference(c)
    assert c.arm == R.EXPECTED_ARMS.get((c.loss, c.L), c.arm), "%s: the restated rule selects the %s arm, the table of threshold lengths names %s" % (
        c.name, c.arm, R.EXPECTED_ARMS.get((c.loss, c.L)))
    pr = Problem(c)
    got = pr.call()
    for k, (g, r, bar) in R.checks(c, got, ref).items():
        ratio = R.worst(g, r, bar)
        key = (_kernel(c), c.arm, c.name, k)
        ROWS[key] = max(ROWS.get(key, 0.0), ratio)
        print("%s [%s]: %s worst error / bar %.4g" % (c.name, c.arm, k, ratio))
        assert ratio <= 1.0, "%s [%s]: %s is outside its bar at %d of %d entries, worst error / bar %.4g" % (
            c.name, c.arm, k, int(R.over(g, r, bar).sum()), np.asarray(g).size, ratio)
    assert not got["grad"][ref["zero"]].any(), "%s: a padded entry of the gradient is not 0" % c.name
    if "order" in ref:
        assert np.array_equal(got["order"], ref["order"]), "%s: order_out differs" % c.name
    if "count" in ref:
        assert got["count"] == ref["count"], "%s: %r selected pairs, the reference has %r" % (c.name, got["count"], ref["count"])
        assert float(got["per_count"].sum()) == ref["count"]
    if isinstance(ref["loss"], float) and np.isnan(ref["loss"]):
        assert np.isnan(got["loss"]), "%s: the mean over an empty selection is not NaN" % c.name
    twice = pr.call()
    for k in got:
        a, b = np.asarray(got[k]), np.asarray(twice[k])
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype.kind == "f" else np.array_equal(a, b), "%s: a second call gives other bits in %s" % (c.name, k)
    for grad, extras in ((False, True), (True, False)):
        other = pr.call(grad=grad, extras=extras)
        assert np.array_equal(_bits(other["loss"]), _bits(got["loss"])), "%s: grad %s / extras %s changes the loss bits" % (c.name, grad, extras)
        if grad:
            assert np.array_equal(_bits(other["grad"]), _bits(got["grad"])), "%s: without the optional outputs the gradient differs" % c.name
    pr.inputs_unchanged()


def _log_rows():
    _log("listwise_contract", dict(seconds_since_import=time.time() - T0,
                                   rows=[dict(kernel=k[0], arm=k[1], case=k[2], output=k[3], worst_error_over_bar=v) for k, v in sorted(ROWS.items())]))


GROUPS = sorted({(c.loss, c.layout, c.L) for c in R.CASES})


@pytest.mark.parametrize("loss,layout,L", [pytest.param(*g, id="%s %s L %d %s" % (g + (R.arm_of(g[0], g[2]),))) for g in GROUPS])
def test_listwise_loss_meets_the_entrywise_contract(loss, layout, L):
    for c in [c for c in R.CASES if (c.loss, c.layout, c.L) == (loss, layout, L)]:
        _contract(c)
    _log_rows()


def test_refusals_return_without_writing():
    _, lib = _libs()
    B, L = 3, 8
    rng = np.random.default_rng(9)
    s, y = _in(rng.standard_normal((B, L))), _in(rng.integers(0, 5, (B, L)))
    perm = Raw(np.arange(L), np.int64, -1)
    cu = Raw([0, 8, 16, 24], np.int32, 0x5A5A5A5A)
    outs = dict(loss=_out(1, 1), per=_out(1, B), grad=_out(B, L), cnt=_out(1, 1))
    order = Raw(np.full(B * L, ORDER_FILL), np.int64, ORDER_FILL)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    wsp = ctypes.c_void_p(ws.data_ptr())
    big = R.MAX_LONG + 1
    D = dict(s=s.ptr, y=y.ptr, B=B, L=L, eps=R.EPS, bd=float(B), loss=outs["loss"].ptr, per=outs["per"].ptr, grad=outs["grad"].ptr, ws=wsp,
             perm=perm.ptr, cu=cu.ptr, scheme=3, red=0, log=0, cnt=outs["cnt"].ptr, order=order.ptr)

    def listnet(**kw):
        a = dict(D, **kw)
        return lib.ltrx_listnet_fwd_bwd(a["s"], a["y"], a["B"], a["L"], a["eps"], -1.0, a["bd"], a["loss"], a["per"], a["grad"], a["ws"], None)

    def listnet_cu(**kw):
        a = dict(D, **kw)
        return lib.ltrx_listnet_fwd_bwd_cu(a["s"], a["y"], a["cu"], None, a["B"], a["L"], a["eps"], a["bd"], a["loss"], a["per"], a["grad"], a["ws"], None)

    def listmle(**kw):
        a = dict(D, **kw)
        return lib.ltrx_listmle_fwd_bwd(a["s"], a["y"], a["perm"], a["B"], a["L"], a["eps"], -1.0, a["bd"], a["loss"], a["per"], a["grad"], a["order"],
                                        a["ws"], None)

    def approx(**kw):
        a = dict(D, **kw)
        return lib.ltrx_approxndcg_fwd_bwd(a["s"], a["y"], a["B"], a["L"], a["eps"], -1.0, 1.0, a["bd"], a["loss"], a["per"], a["grad"], a["ws"], None)

    def approx_cu(**kw):
        a = dict(D, **kw)
        return lib.ltrx_approxndcg_fwd_bwd_cu(a["s"], a["y"], a["cu"], None, a["B"], a["L"], a["eps"], 1.0, a["bd"], a["loss"], a["per"], a["grad"],
                                              a["ws"], None)

    def lam(**kw):
        a = dict(D, **kw)
        return lib.ltrx_lambdaloss_fwd_bwd(a["s"], a["y"], a["B"], a["L"], a["eps"], -1.0, a["scheme"], 0, 1.0, 10.0, a["red"], a["log"], None,
                                           a["loss"], a["cnt"], a["grad"], a["order"], a["ws"], None)

    def lam_cu(**kw):
        a = dict(D, **kw)
        return lib.ltrx_lambdaloss_fwd_bwd_cu(a["s"], a["y"], a["cu"], None, a["B"], a["L"], a["eps"], a["scheme"], 0, 1.0, 10.0, a["red"], a["log"],
                                              None, a["loss"], a["cnt"], a["grad"], a["order"], a["ws"], None)

    common = (dict(s=None), dict(y=None), dict(loss=None), dict(ws=None), dict(B=0), dict(B=-2), dict(L=0))
    for fn in (listnet, listnet_cu, listmle, approx, approx_cu, lam, lam_cu):
        for kw in common:
            assert fn(**kw) == EINVAL, (fn.__name__, sorted(kw))
        assert fn(L=big) == EUNSUPPORTED, fn.__name__
    for fn in (listnet, listnet_cu, listmle, approx, approx_cu):
        assert fn(bd=0.0) == EINVAL and fn(bd=-1.0) == EINVAL, fn.__name__
    for fn in (listnet_cu, approx_cu, lam_cu):
        assert fn(cu=None) == EINVAL, fn.__name__
    assert listmle(perm=None) == EINVAL
    for fn in (lam, lam_cu):
        for kw in (dict(eps=0.0), dict(eps=-1e-10), dict(scheme=-1), dict(scheme=8), dict(red=2), dict(log=-1)):
            assert fn(**kw) == EINVAL, (fn.__name__, sorted(kw))
    torch.cuda.synchronize()
    for name, wnd in outs.items():
        wnd.unchanged("a refused call wrote " + name)
    order.unchanged("a refused call wrote order_out")
    for wnd in (s, y, perm, cu):
        wnd.unchanged("a refused call wrote an input")
    assert not bool(ws.any()), "a refused call wrote its workspace"
    for loss in R.NARR:
        assert getattr(lib, "ltrx_%s_workspace_bytes" % loss)(0, 0) == R.per_floats(loss, 0) * 4
