"""The contract of the loss kernels of allrank_amd/csrc/ltrx_pointpair.hip, -m gpu: ltrx_ranknet_fwd_bwd (three weight modes),
ltrx_bce_fwd_bwd (bce and ordinal), ltrx_pointwise_rmse_fwd_bwd and ltrx_binary_listnet_fwd_bwd, with ltrx_ratio_finalize_kernel and
ltrx_scale_by_device_kernel behind the first two.

One call through the C ABI per comparison and one assertion for EVERY entry of every output: |kernel - fp64 reference| <= bar for every
gradient entry, the per-slate values at the head of the workspace and the loss; padded entries exactly 0; the per-slate counts and
pair_count_out / count_out exact; a batch without pairs gives a NaN loss and a gradient of exactly 0; an exactly fitted rmse slate gives
rmse 0 and a NaN gradient on its valid items, an all-padded one a NaN rmse and loss.  The references, the derivation of the bars, the
defect models and the case tables are in tests/pointpair_ref.py; tests/test_pointpair_ref_cpu.py is the evidence that the bars bite.

Around every window the buffers hold sentinels (NaN around outputs, 3e37 around inputs, 0xA5 behind a workspace of exactly
ltrx_*_workspace_bytes, NaN inside it before the call) that must survive; inputs must be unchanged; a second identical call gives the
same bits; calls with grad_out = NULL and pair_count_out / count_out = NULL give the same loss bits.  The worst error / bar of every
(kernel, case, output) is logged as parity_pointpair_contract.json."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import pointpair_ref as R
from tests.test_gpu_gemm_contract import EINVAL, EUNSUPPORTED, GARBAGE, Win
from tests.test_gpu_parity import DEV, _log

pytestmark = pytest.mark.gpu

F = np.float32
TAIL = 4096
ROWS = {}
T0 = time.time()


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


KERNEL_OF = (("ranknet", "ltrx_ranknet_kernel"), ("bce", "ltrx_bce_kernel"), ("ordinal", "ltrx_bce_kernel"),
             ("pointwise_rmse", "ltrx_pointwise_rmse_kernel"), ("binary_listNet", "ltrx_binary_listnet_kernel"))


def _log_rows():
    """every test function rewrites the log from the shared ROWS; the kernel of a row is named by its case, here alone"""
    kernel = lambda case: [k for pre, k in KERNEL_OF if case.startswith(pre)][0]      # noqa: E731
    _log("pointpair_contract", dict(seconds_since_import=time.time() - T0,
                                    rows=[dict(kernel=kernel(k[0]), case=k[0], output=k[1], worst_error_over_bar=v) for k, v in sorted(ROWS.items())]))


class Problem(object):
    def __init__(self, c):
        self.c, self.bt = c, R.inputs(c)
        self.ins = dict(s=_in(self.bt.s), y=_in(self.bt.y))
        if c.ext is not None:
            self.ins["ext"] = _in([[c.ext]])

    def call(self, grad=True, count=True):
        _, lib = _libs()
        c, bt, ins = self.c, self.bt, self.ins
        B, L = bt.B, bt.L
        what = "%s (grad %s, count %s)" % (c.name, grad, count)
        nws = lib.ltrx_ranknet_workspace_bytes(B, L)
        assert nws == R.workspace_bytes(B), "%s: the library sizes its workspace as %d bytes, the restated rule as %d" % (c.name, nws, R.workspace_bytes(B))
        ws = torch.full((nws + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
        ws[nws:] = 0xA5
        loss, g, cnt = _out(1, 1), (_out(B, L) if grad else None), (_out(1, 1) if count else None)
        P = lambda x: x.ptr if x is not None else None      # noqa: E731
        ext = ins["ext"].ptr if c.ext is not None else None
        _run(what, lambda: lib.ltrx_ranknet_fwd_bwd(ins["s"].ptr, ins["y"].ptr, B, L, float(R.PAD), c.mode, ext, loss.ptr, P(cnt), P(g),
                                                    ctypes.c_void_p(ws.data_ptr()), None))
        assert bool((ws[nws:] == 0xA5).all()), "%s: wrote behind its %d-byte workspace" % (what, nws)
        head = ws[:8 * B].cpu().numpy().view(F)
        out = dict(loss=loss.fetch(what + " loss")[0, 0], per=head[:B].copy(), per_count=head[B:].copy())
        if grad:
            out["grad"] = g.fetch(what + " grad")
        if count:
            out["count"] = float(cnt.fetch(what + " pair count")[0, 0])
        return out

    def inputs_unchanged(self):
        for name, wnd in self.ins.items():
            wnd.unchanged("%s %s" % (self.c.name, name))


def _contract(c):
    ref = R.reference(c)
    pr = Problem(c)
    got = pr.call()
    for k, (g, r, bar) in R.checks(c, got, ref).items():
        ratio = R.worst(g, r, bar)
        ROWS[(c.name, k)] = max(ROWS.get((c.name, k), 0.0), ratio)
        print("%s: %s worst error / bar %.4g" % (c.name, k, ratio))
        assert ratio <= 1.0, "%s: %s is outside its bar at %d of %d entries, worst error / bar %.4g" % (
            c.name, k, int(R.over(g, r, bar).sum()), np.asarray(g).size, ratio)
    assert R.exact_ok(c, got, ref), "%s: an exact output (padded zeros, the counts, a slate or batch without pairs) differs" % c.name
    twice = pr.call()
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(twice[k])), "%s: a second call gives other bits in %s" % (c.name, k)
    for grad, count in ((False, True), (True, False)):
        other = pr.call(grad=grad, count=count)
        assert np.array_equal(_bits(other["loss"]), _bits(got["loss"])), "%s: grad %s / count %s changes the loss bits" % (c.name, grad, count)
        assert np.array_equal(_bits(other["per"]), _bits(got["per"])) and np.array_equal(_bits(other["per_count"]), _bits(got["per_count"]))
        if grad:
            assert np.array_equal(_bits(other["grad"]), _bits(got["grad"])), "%s: pair_count_out = NULL changes the gradient" % c.name
    pr.inputs_unchanged()


@pytest.mark.parametrize("L", sorted({c.L for c in R.CASES}))
def test_ranknet_meets_the_entrywise_contract(L):
    t0 = time.time()
    for c in [c for c in R.CASES if c.L == L]:
        _contract(c)
    _log_rows()
    print("ranknet L %d: %.2f s" % (L, time.time() - t0))


def test_refusals_return_without_writing():
    _, lib = _libs()
    B, L = 3, 8
    rng = np.random.default_rng(9)
    s, y = _in(rng.standard_normal((B, L))), _in(rng.integers(0, 5, (B, L)))
    outs = dict(loss=_out(1, 1), cnt=_out(1, 1), grad=_out(B, L))
    ws = torch.zeros(1 << 12, dtype=torch.uint8, device=DEV)
    D = dict(s=s.ptr, y=y.ptr, B=B, L=L, mode=0, loss=outs["loss"].ptr, ws=ctypes.c_void_p(ws.data_ptr()))

    def ranknet(**kw):
        a = dict(D, **kw)
        return lib.ltrx_ranknet_fwd_bwd(a["s"], a["y"], a["B"], a["L"], -1.0, a["mode"], None, a["loss"], outs["cnt"].ptr, outs["grad"].ptr, a["ws"], None)

    for kw in (dict(s=None), dict(y=None), dict(loss=None), dict(ws=None), dict(B=0), dict(B=-2), dict(L=0), dict(L=-1), dict(mode=-1), dict(mode=3)):
        assert ranknet(**kw) == EINVAL, sorted(kw)
    assert ranknet(L=R.MAX_L + 1) == EUNSUPPORTED
    torch.cuda.synchronize()
    for name, wnd in outs.items():
        wnd.unchanged("a refused call wrote " + name)
    s.unchanged("a refused call wrote an input"), y.unchanged("a refused call wrote an input")
    assert not bool(ws.any()), "a refused call wrote its workspace"
    assert lib.ltrx_ranknet_workspace_bytes(0, 0) == R.workspace_bytes(0)


def test_ranknet_wrappers_equal_the_abi_call_bit_for_bit():
    """losses.rankNet, rankNet_weightByGTDiff and rankNet_weightByGTDiff_pow are this ABI call: the same loss and gradient bits"""
    from allrank_amd import losses as E
    fns = {0: E.rankNet, 1: E.rankNet_weightByGTDiff, 2: E.rankNet_weightByGTDiff_pow}
    for mode, fn in fns.items():
        c = [c for c in R.CASES if c.L == 257 and c.scale == 30 and c.mode == mode and c.ext is None][0]
        bt = R.inputs(c)
        got = Problem(c).call()
        sp = torch.tensor(bt.s, device=DEV, requires_grad=True)
        loss = fn(sp, torch.tensor(bt.y, device=DEV))
        loss.backward()
        assert np.array_equal(_bits(loss.detach().cpu().numpy()), _bits(got["loss"])), c.name
        assert np.array_equal(_bits(sp.grad.cpu().numpy()), _bits(got["grad"])), c.name


# ---------------------------------------------------------------------------------------------------------------------------------
# bce / ordinal (ltrx_bce_fwd_bwd): the same contract; the B = 64, L = 2049, n = 4 case is the second grid-stride trip of
# ltrx_scale_by_device_kernel, L = 2049 and 5000 are above the limit of the LDS-resident losses and must work
# ---------------------------------------------------------------------------------------------------------------------------------
class BceProblem(object):
    def __init__(self, c):
        self.c = c
        self.y, self.p = R.bce_inputs(c)
        self.ins = dict(y=_in(self.y), p=_in(self.p.reshape(c.B, -1)))
        if c.ext is not None:
            self.ins["ext"] = _in([[c.ext]])

    def call(self, grad=True, count=True):
        _, lib = _libs()
        c, ins = self.c, self.ins
        B, L, cols = c.B, c.L, c.L * max(c.n, 1)
        what = "%s (grad %s, count %s)" % (c.name, grad, count)
        nws = lib.ltrx_bce_workspace_bytes(B, L, c.n)
        assert nws == R.workspace_bytes(B), "%s: the library sizes its workspace as %d bytes, the restated rule as %d" % (c.name, nws, R.workspace_bytes(B))
        ws = torch.full((nws + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
        ws[nws:] = 0xA5
        loss, g, cnt = _out(1, 1), (_out(B, cols) if grad else None), (_out(1, 1) if count else None)
        P = lambda x: x.ptr if x is not None else None      # noqa: E731
        ext = ins["ext"].ptr if c.ext is not None else None
        _run(what, lambda: lib.ltrx_bce_fwd_bwd(ins["p"].ptr, ins["y"].ptr, B, L, c.n, float(R.PAD), ext, loss.ptr, P(cnt), P(g),
                                                ctypes.c_void_p(ws.data_ptr()), None))
        assert bool((ws[nws:] == 0xA5).all()), "%s: wrote behind its %d-byte workspace" % (what, nws)
        head = ws[:8 * B].cpu().numpy().view(F)
        out = dict(loss=loss.fetch(what + " loss")[0, 0], per=head[:B].copy(), per_count=head[B:].copy())
        if grad:
            out["grad"] = g.fetch(what + " grad").reshape(self.p.shape)
        if count:
            out["count"] = float(cnt.fetch(what + " count")[0, 0])
        return out


def _bce_contract(c):
    ref = R.bce_reference(c)
    pr = BceProblem(c)
    got = pr.call()
    for k, (g, r, bar) in R.checks(c, got, ref).items():
        ratio = R.worst(g, r, bar)
        ROWS[(c.name, k)] = max(ROWS.get((c.name, k), 0.0), ratio)
        print("%s: %s worst error / bar %.4g" % (c.name, k, ratio))
        assert ratio <= 1.0, "%s: %s is outside its bar at %d of %d entries, worst error / bar %.4g" % (
            c.name, k, int(R.over(g, r, bar).sum()), np.asarray(g).size, ratio)
    assert R.exact_ok(c, got, ref), "%s: an exact output (padded zeros, the counts) differs" % c.name
    twice = pr.call()
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(twice[k])), "%s: a second call gives other bits in %s" % (c.name, k)
    for grad, count in ((False, True), (True, False)):
        other = pr.call(grad=grad, count=count)
        assert np.array_equal(_bits(other["loss"]), _bits(got["loss"])), "%s: grad %s / count %s changes the loss bits" % (c.name, grad, count)
        if grad:
            assert np.array_equal(_bits(other["grad"]), _bits(got["grad"])), "%s: count_out = NULL changes the gradient" % c.name
    for name, wnd in pr.ins.items():
        wnd.unchanged("%s %s" % (c.name, name))


@pytest.mark.parametrize("L", sorted({c.L for c in R.BCE_CASES}))
def test_bce_and_ordinal_meet_the_entrywise_contract(L):
    t0 = time.time()
    for c in [c for c in R.BCE_CASES if c.L == L]:
        _bce_contract(c)
    _log_rows()
    print("bce / ordinal L %d: %.2f s" % (L, time.time() - t0))


def test_bce_refusals_return_without_writing():
    _, lib = _libs()
    B, L = 3, 8
    rng = np.random.default_rng(9)
    p, y = _in(rng.uniform(0.1, 0.9, (B, L))), _in(rng.integers(0, 2, (B, L)))
    outs = dict(loss=_out(1, 1), cnt=_out(1, 1), grad=_out(B, L))
    ws = torch.zeros(1 << 12, dtype=torch.uint8, device=DEV)
    D = dict(p=p.ptr, y=y.ptr, B=B, L=L, n=0, loss=outs["loss"].ptr, ws=ctypes.c_void_p(ws.data_ptr()))

    def bce(**kw):
        a = dict(D, **kw)
        return lib.ltrx_bce_fwd_bwd(a["p"], a["y"], a["B"], a["L"], a["n"], -1.0, None, a["loss"], outs["cnt"].ptr, outs["grad"].ptr, a["ws"], None)

    for kw in (dict(p=None), dict(y=None), dict(loss=None), dict(ws=None), dict(B=0), dict(B=-2), dict(L=0), dict(L=-1), dict(n=-1)):
        assert bce(**kw) == EINVAL, sorted(kw)
    torch.cuda.synchronize()
    for name, wnd in outs.items():
        wnd.unchanged("a refused call wrote " + name)
    p.unchanged("a refused call wrote an input"), y.unchanged("a refused call wrote an input")
    assert not bool(ws.any()), "a refused call wrote its workspace"


def test_bce_and_ordinal_wrappers_equal_the_abi_call_bit_for_bit():
    """losses.bce and losses.ordinal are this ABI call: the same loss and gradient bits"""
    from allrank_amd import losses as E
    for n in (0, 3):
        c = [c for c in R.BCE_CASES if c.L == 257 and c.n == n and c.ext is None][0]
        y, p = R.bce_inputs(c)
        got = BceProblem(c).call()
        pt = torch.tensor(p, device=DEV, requires_grad=True)
        loss = E.ordinal(pt, torch.tensor(y, device=DEV), n) if n else E.bce(pt, torch.tensor(y, device=DEV))
        loss.backward()
        assert np.array_equal(_bits(loss.detach().cpu().numpy()), _bits(got["loss"])), c.name
        assert np.array_equal(_bits(pt.grad.cpu().numpy()), _bits(got["grad"])), c.name


# ---------------------------------------------------------------------------------------------------------------------------------
# pointwise_rmse and binary_listNet: no count, the divisor is the batch size; the per-slate values are the B floats of the workspace
# ---------------------------------------------------------------------------------------------------------------------------------
class PlainProblem(object):
    """loss "rmse": (y, p) of an RCase; "blistnet": the Batch of an LCase"""

    def __init__(self, loss, c):
        self.loss, self.c = loss, c
        if loss == "rmse":
            self.y, self.x = R.rmse_inputs(c)
        else:
            bt = R.blistnet_inputs(c)
            self.y, self.x = bt.y, bt.s
        self.ins = dict(y=_in(self.y), x=_in(self.x))

    def call(self, grad=True):
        _, lib = _libs()
        c, ins = self.c, self.ins
        B, L = self.y.shape
        what = "%s (grad %s)" % (c.name, grad)
        sizer = lib.ltrx_pointwise_rmse_workspace_bytes if self.loss == "rmse" else lib.ltrx_binary_listnet_workspace_bytes
        nws = sizer(B, L)
        assert nws == 4 * B, "%s: the library sizes its workspace as %d bytes, the restated rule as %d" % (c.name, nws, 4 * B)
        ws = torch.full((nws + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
        ws[nws:] = 0xA5
        loss, g = _out(1, 1), (_out(B, L) if grad else None)
        gp, wsp = (g.ptr if grad else None), ctypes.c_void_p(ws.data_ptr())
        if self.loss == "rmse":
            fn = lambda: lib.ltrx_pointwise_rmse_fwd_bwd(ins["x"].ptr, ins["y"].ptr, B, L, float(c.levels), float(R.PAD), float(B), loss.ptr, gp, wsp, None)   # noqa: E731
        else:
            fn = lambda: lib.ltrx_binary_listnet_fwd_bwd(ins["x"].ptr, ins["y"].ptr, B, L, R.EPS, float(R.PAD), float(B), loss.ptr, gp, wsp, None)   # noqa: E731
        _run(what, fn)
        assert bool((ws[nws:] == 0xA5).all()), "%s: wrote behind its %d-byte workspace" % (what, nws)
        out = dict(loss=loss.fetch(what + " loss")[0, 0], per=ws[:4 * B].cpu().numpy().view(F).copy())
        if grad:
            out["grad"] = g.fetch(what + " grad")
        return out


def _plain_contract(loss, c):
    ref = (R.rmse_reference if loss == "rmse" else R.blistnet_reference)(c)
    pr = PlainProblem(loss, c)
    got = pr.call()
    for k, (g, r, bar) in R.plain_checks(got, ref).items():
        ratio = R.worst(g, r, bar)
        ROWS[(c.name, k)] = max(ROWS.get((c.name, k), 0.0), ratio)
        print("%s: %s worst error / bar %.4g" % (c.name, k, ratio))
        assert ratio <= 1.0, "%s: %s is outside its bar at %d of %d entries, worst error / bar %.4g" % (
            c.name, k, int(R.over(g, r, bar).sum()), np.asarray(g).size, ratio)
    assert R.plain_exact_ok(got, ref), "%s: an exact output (padded zeros, a fitted, zero-label or all-padded slate) differs" % c.name
    twice = pr.call()
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(twice[k])), "%s: a second call gives other bits in %s" % (c.name, k)
    other = pr.call(grad=False)
    assert np.array_equal(_bits(other["loss"]), _bits(got["loss"])) and np.array_equal(_bits(other["per"]), _bits(got["per"])), (
        "%s: grad_out = NULL changes the loss bits" % c.name)
    for name, wnd in pr.ins.items():
        wnd.unchanged("%s %s" % (c.name, name))


PLAIN_GROUPS = sorted({("rmse", c.L) for c in R.RMSE_CASES} | {("blistnet", c.L) for c in R.BLISTNET_CASES})


@pytest.mark.parametrize("loss,L", PLAIN_GROUPS)
def test_rmse_and_binary_listnet_meet_the_entrywise_contract(loss, L):
    t0 = time.time()
    for c in [c for c in (R.RMSE_CASES if loss == "rmse" else R.BLISTNET_CASES) if c.L == L]:
        _plain_contract(loss, c)
    _log_rows()
    print("%s L %d: %.2f s" % (loss, L, time.time() - t0))


def test_rmse_and_binary_listnet_refusals_return_without_writing():
    _, lib = _libs()
    B, L = 3, 8
    rng = np.random.default_rng(9)
    x, y = _in(rng.uniform(0.1, 0.9, (B, L))), _in(rng.integers(0, 5, (B, L)))
    outs = dict(loss=_out(1, 1), grad=_out(B, L))
    ws = torch.zeros(1 << 12, dtype=torch.uint8, device=DEV)
    D = dict(x=x.ptr, y=y.ptr, B=B, L=L, bd=float(B), loss=outs["loss"].ptr, ws=ctypes.c_void_p(ws.data_ptr()))

    def rmse(**kw):
        a = dict(D, **kw)
        return lib.ltrx_pointwise_rmse_fwd_bwd(a["x"], a["y"], a["B"], a["L"], 4.0, -1.0, a["bd"], a["loss"], outs["grad"].ptr, a["ws"], None)

    def blistnet(**kw):
        a = dict(D, **kw)
        return lib.ltrx_binary_listnet_fwd_bwd(a["x"], a["y"], a["B"], a["L"], R.EPS, -1.0, a["bd"], a["loss"], outs["grad"].ptr, a["ws"], None)

    for fn in (rmse, blistnet):
        for kw in (dict(x=None), dict(y=None), dict(loss=None), dict(ws=None), dict(B=0), dict(B=-2), dict(L=0), dict(L=-1), dict(bd=0.0), dict(bd=-1.0)):
            assert fn(**kw) == EINVAL, (fn.__name__, sorted(kw))
    assert blistnet(L=R.MAX_L + 1) == EUNSUPPORTED
    torch.cuda.synchronize()
    for name, wnd in outs.items():
        wnd.unchanged("a refused call wrote " + name)
    x.unchanged("a refused call wrote an input"), y.unchanged("a refused call wrote an input")
    assert not bool(ws.any()), "a refused call wrote its workspace"
    assert lib.ltrx_pointwise_rmse_workspace_bytes(0, 0) == 0 and lib.ltrx_binary_listnet_workspace_bytes(-1, 3) == 0


def test_rmse_and_binary_listnet_wrappers_equal_the_abi_call_bit_for_bit():
    """losses.pointwise_rmse and losses.binary_listNet are these ABI calls: the same loss and gradient bits (NaN entries included)"""
    from allrank_amd import losses as E
    for loss, c in (("rmse", [c for c in R.RMSE_CASES if c.L == 257 and c.levels == 4][0]),
                    ("blistnet", [c for c in R.BLISTNET_CASES if c.L == 257 and c.scale == 30][0])):
        pr = PlainProblem(loss, c)
        got = pr.call()
        xt = torch.tensor(pr.x, device=DEV, requires_grad=True)
        yt = torch.tensor(pr.y, device=DEV)
        out = E.pointwise_rmse(xt, yt, c.levels) if loss == "rmse" else E.binary_listNet(xt, yt)
        out.backward()
        assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(got["loss"])), c.name
        assert np.array_equal(_bits(xt.grad.cpu().numpy()), _bits(got["grad"])), c.name
