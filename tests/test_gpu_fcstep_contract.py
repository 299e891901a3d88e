"""The stagewise entrywise contract of the slate-resident FC + ListNet step (allrank_amd/csrc/ltrx_fcstep.hip), -m gpu.

Both entry points, ltrx_fc_listnet_step and ltrx_fc_linear_listnet_step, are called through the C ABI on every case of
tests/fcstep_ref.py's table (the compute-unit count is the device's), and EVERY entry of every output is held to its bar: hidden,
the ReLU pattern, scores, d loss / d scores, the loss, dW1, db1, dw_out, db_out, the H4 padding slots (exactly 0), and with Adam the
parameters, both moments and the step count -- each stage against an fp64 reference fed with the kernel's own upstream output.  The
references, the term-by-term derivation of the bars, the defect models and the table are in tests/fcstep_ref.py;
tests/test_fcstep_ref_cpu.py is the evidence that the bars bite (an fp32 transcription inside every bar, every defect outside).

Around every window the buffers hold sentinels (NaN around outputs, 3e37 around inputs); the workspace is NaN-filled (an unwritten
partial entry would show in the gradient), must stay untouched from the extent the nwg workgroups may write up to *_workspace_bytes,
and holds 0xA5 behind it.  x, y and -- with Adam off -- params must be unchanged.  hidden_out = NULL and, separately, dscores = NULL
(the forms the engine uses) give bit-identical scores, gradients and loss; so does a repeated call.

Adam: the header promises ltrx_adam_step's update rule, and the three kernels spell it with the same expressions in the same order.
The fused update is also compared with ltrx_adam_step on the same gradients bit for bit: the bits DIFFER (a tenth to a fifth of the
entries, with L2 and with AdamW alike), because the sources part below the level they fix: each of gr = g s + l2 p, m' = b1 m
+ (1 - b1) gr, v' = b2 v + (1 - b2) gr gr and p' = p shrink - ss (m' / den) is a sum of two products, of which the compiler fuses one
into the addition, and it chooses per kernel (ltrx_adam_kernel works on float4 members with a run-time grad_scale, the fused kernels on
vector elements with the literal 1.0f, which folds away).  step_ref.adam_bar counts every product as rounded and covers either
choice: it is the assertion; the number of differing entries is logged.

The worst error / bar per kernel and stage is written to parity_fcstep_contract.json."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fcstep_ref as R
from tests.test_gpu_gemm_contract import EINVAL, EUNSUPPORTED, GARBAGE, Win
from tests.test_gpu_parity import DEV, _log

pytestmark = pytest.mark.gpu

F = np.float32
TAIL = 4096
ROWS, ADAM_BITS = {}, {}


def _libs():
    from allrank_amd import _lib as LB
    return LB, LB.lib()


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _in(data):
    data = np.atleast_2d(np.asarray(data, F))
    return Win(data.shape, data.shape[1], 4, GARBAGE, data)


def _io(data):
    """a buffer the call may update (params, moments, the step count): NaN around it"""
    data = np.atleast_2d(np.asarray(data, F))
    return Win(data.shape, data.shape[1], 4, np.nan, data)


def _out(rows, cols):
    return Win((rows, cols), cols, 4, np.nan)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


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


class Workspace(object):
    def __init__(self, kind, B, Fn, H, cus, nbytes):
        assert nbytes == R.ws_bytes(kind, B, Fn, H)
        self.n, self.used = nbytes, R.ws_used(kind, B, Fn, H, cus)
        assert self.used <= self.n
        self.buf = torch.full((nbytes + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
        self.buf[nbytes:] = 0xA5
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr())

    def check(self, what):
        assert bool((self.buf[self.n:] == 0xA5).all()), "%s: wrote behind its %d-byte workspace" % (what, self.n)
        assert bool((self.buf[self.used:self.n] == 0xFF).all()), "%s: wrote behind the %d bytes its workgroups own" % (what, self.used)

    def untouched(self):
        return bool((self.buf[:self.n] == 0xFF).all()) and bool((self.buf[self.n:] == 0xA5).all())


class Problem(object):
    """one case on the device"""

    def __init__(self, c):
        self.cus = _cus()
        self.c = R.resolve(c, self.cus)
        self.X = R.inputs(self.c, self.cus)
        X = self.X
        self.B, self.L, self.Fn, self.H = X["B"], c.L, c.F, c.H
        self.x, self.y = _in(X["x"].reshape(self.B * self.L, self.Fn)), _in(X["y"])
        self.lay = R.layout(self.Fn, self.H)

    def call(self, hidden=True, dscores=True, adam=None, **over):
        """one call with fresh output / state windows; returns (got, windows)"""
        _, lib = _libs()
        c, X, B, L, Fn, H = self.c, self.X, self.B, self.L, self.Fn, self.H
        adam = c.adam if adam is None else adam
        nflat = self.lay[4]
        W = dict(params=_io(X["params"]), scores=_out(B, L), dsc=_out(B, L), hid=_out(B * L, H), loss=_out(1, 1), grads=_out(1, nflat),
                 m=_io(X["m"]), v=_io(X["v"]), step=_io([c.t0]))
        if c.kind == "fc":
            nws = lib.ltrx_fc_listnet_workspace_bytes(B, L, Fn, H, nflat)
        else:
            nws = lib.ltrx_fc_linear_listnet_workspace_bytes(B, Fn)
        ws = Workspace(c.kind, B, Fn, H, self.cus, nws)
        a = dict(x=self.x.ptr, y=self.y.ptr, B=B, L=L, F=Fn, H=H, act=c.act, params=W["params"].ptr, offs=self.lay, eps=c.eps, pad=R.PAD,
                 div=c.div, scores=W["scores"].ptr, dsc=W["dsc"].ptr if dscores else None, hid=W["hid"].ptr if hidden else None,
                 loss=W["loss"].ptr, grads=W["grads"].ptr, m=W["m"].ptr if adam else None, v=W["v"].ptr if adam else None,
                 step=W["step"].ptr if adam else None, decoupled=int(adam == "adamw"), ws=ws.ptr)
        a.update(over)
        opt = (a["m"], a["v"], a["step"], R.ADAM["lr"], R.ADAM["b1"], R.ADAM["b2"], R.ADAM["eps"], R.ADAM["wd"], a["decoupled"], a["ws"], None)
        head = (a["x"], a["y"], a["B"], a["L"], a["F"], a["H"])
        mid = (a["params"],) + tuple(a["offs"]) + (a["eps"], a["pad"], a["div"], a["scores"], a["dsc"])
        if c.kind == "fc":
            fn = lambda: lib.ltrx_fc_listnet_step(*head, a["act"], *mid, a["hid"], a["loss"], a["grads"], *opt)      # noqa: E731
        else:
            fn = lambda: lib.ltrx_fc_linear_listnet_step(*head, *mid, a["loss"], a["grads"], *opt)                   # noqa: E731
        W["ws"] = ws
        return fn, W, adam

    def run(self, what, **kw):
        c, B, L, H = self.c, self.B, self.L, self.H
        fn, W, adam = self.call(**kw)
        _run(what, fn)
        W["ws"].check(what)
        got = dict(scores=W["scores"].fetch(what + " scores"), loss=W["loss"].fetch(what + " loss")[0, 0], grads=W["grads"].fetch(what + " grads")[0])
        if kw.get("dscores", True):
            got["dscores"] = W["dsc"].fetch(what + " dscores")
        else:
            W["dsc"].unchanged(what + " dscores (NULL)")
        if c.kind == "fc" and kw.get("hidden", True):
            got["hidden"] = W["hid"].fetch(what + " hidden_out").reshape(B, L, H)
        else:
            W["hid"].unchanged(what + " hidden_out (NULL)")
        if adam:
            got.update(params=W["params"].fetch(what + " params")[0], exp_avg=W["m"].fetch(what + " exp_avg")[0],
                       exp_avg_sq=W["v"].fetch(what + " exp_avg_sq")[0], step=W["step"].fetch(what + " step_count")[0, 0])
        else:
            for name in ("params", "m", "v", "step"):
                W[name].unchanged("%s %s (Adam off)" % (what, name))
        self.x.unchanged(what + " x")
        self.y.unchanged(what + " y")
        return got


def _assert_stages(c, X, got, cus, kernel, record=True):
    bad = []
    for name, a, r, b in R.stages(c, X, got, cus):
        ratio = R.worst(a, r, b)
        if record:
            for key in ((kernel, name), (kernel, name, c.name)):
                ROWS[key] = max(ROWS.get(key, 0.0), ratio)
        print("%s, %s: %s worst error / bar %.4g" % (kernel, c.name, name, ratio))
        if not ratio <= 1.0:
            bad.append("%s is outside its bar at %d of %d entries, worst error / bar %.4g" % (name, int(R.over(a, r, b).sum()), np.asarray(a).size, ratio))
    assert not bad, "%s, %s: %s" % (kernel, c.name, "; ".join(bad))


def _log_rows():
    per = [dict(kernel=k[0], stage=k[1], worst_error_over_bar=v) for k, v in sorted(ROWS.items()) if len(k) == 2]
    cases = [dict(kernel=k[0], stage=k[1], case=k[2], worst_error_over_bar=v) for k, v in sorted(ROWS.items()) if len(k) == 3]
    _log("fcstep_contract", dict(per_kernel_and_stage=per, adam_entries_differing_from_ltrx_adam_step=ADAM_BITS, cases=cases))


def _adam_step_bits(pr, got):
    """ltrx_adam_step on the gradients the fused step wrote, from the same state"""
    _, lib = _libs()
    c, X = pr.c, pr.X
    n = pr.lay[4]
    P, G, M, V, S = _io(X["params"]), _in(got["grads"]), _io(X["m"]), _io(X["v"]), _io([c.t0])
    _run("ltrx_adam_step", lambda: lib.ltrx_adam_step(P.ptr, G.ptr, M.ptr, V.ptr, n, R.ADAM["lr"], R.ADAM["b1"], R.ADAM["b2"], R.ADAM["eps"],
                                                      R.ADAM["wd"], int(c.adam == "adamw"), S.ptr, 1.0, None, None))
    diff = sum(int((_bits(a.fetch("ltrx_adam_step")[0]) != _bits(got[k])).sum()) for a, k in ((P, "params"), (M, "exp_avg"), (V, "exp_avg_sq")))
    ADAM_BITS[c.name] = diff
    print("%s: %d of %d entries of the fused update differ from ltrx_adam_step's bits" % (c.name, diff, 3 * n))


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in R.CASES])
def test_fc_step_meets_the_stagewise_contract(c):
    pr = Problem(c)
    kernel = R.kernel_name(c)
    got = pr.run(c.name)
    _assert_stages(pr.c, pr.X, got, pr.cus, kernel)
    if c.adam:
        _adam_step_bits(pr, got)
    same = ("scores", "grads", "loss") + (("params", "exp_avg", "exp_avg_sq") if c.adam else ())
    forms = [("a repeated call", dict()), ("dscores = NULL", dict(dscores=False))] + ([("hidden_out = NULL", dict(hidden=False))] if c.kind == "fc" else [])
    for what, kw in forms:
        twice = pr.run("%s, %s" % (c.name, what), **kw)
        for k in same + (("dscores", "hidden") if not kw else ()):
            if k in got:
                assert np.array_equal(_bits(got[k]), _bits(twice[k])), "%s: %s gives other bits of %s" % (c.name, what, k)
    _log_rows()


def test_the_comparison_tells_a_dropped_split_term_and_a_dropped_slate():
    """negative controls: the device's outputs pass, and the transcription with x_hi dh_lo dropped from the weight gradient (a small case)
    and with every slate after a workgroup's first dropped (cus + 1 slates) fails, through the same comparison code"""
    small = [c for c in R.CASES if c.kind == "fc" and (c.B, c.L, c.F) == (3, 17, 36)][0]
    many = [c for c in R.CASES if c.kind == "fc" and c.B == (1, 1) and c.F == 36][0]
    for c, wrong, stage in ((small, "no_xh_dhl", "dW1"), (many, "first_slate_only", "dW1")):
        pr = Problem(c)
        assert R.applies(pr.c, pr.X, pr.cus, wrong) is None
        _assert_stages(pr.c, pr.X, pr.run(c.name), pr.cus, R.kernel_name(c), record=False)
        with pytest.raises(AssertionError, match=stage + " is outside its bar"):
            _assert_stages(pr.c, pr.X, R.transcribe(pr.c, pr.X, pr.cus, wrong), pr.cus, R.kernel_name(c), record=False)


@pytest.mark.parametrize("kind", ["fc", "lin"])
def test_refusals_return_the_documented_code_without_writing(kind):
    c = [c for c in R.CASES if c.kind == kind and c.adam and isinstance(c.B, int)][0]
    pr = Problem(c)
    Fn, H = pr.Fn, pr.H
    lay = pr.lay
    off = lambda p: ctypes.c_void_p(p.value + 4)      # noqa: E731
    refusals = [("L 257", dict(L=257), EUNSUPPORTED), ("F 148", dict(F=148, offs=R.layout(148, H)), EUNSUPPORTED),
                ("F 134", dict(F=134, offs=R.layout(134, H)), EUNSUPPORTED), ("H 112", dict(H=112, offs=R.layout(Fn, 112)), EUNSUPPORTED),
                ("a wrong offset", dict(offs=(lay[0], lay[1] + 4) + lay[2:]), EINVAL), ("off_w1 != 0", dict(offs=(4,) + lay[1:]), EINVAL),
                ("a wrong nflat", dict(offs=lay[:4] + (lay[4] + 4,)), EINVAL), ("batch_divisor 0", dict(div=0.0), EINVAL),
                ("batch_divisor NaN", dict(div=float("nan")), EINVAL), ("B 0", dict(B=0), EINVAL), ("exp_avg without exp_avg_sq", dict(v=None), EINVAL),
                ("exp_avg without step_count", dict(step=None), EINVAL), ("x = NULL", dict(x=None), EINVAL), ("ws = NULL", dict(ws=None), EINVAL)]
    if kind == "fc":
        refusals += [("act 2", dict(act=2), EINVAL), ("act -1", dict(act=-1), EINVAL)]
    for what, kw, code in refusals:
        fn, W, _ = pr.call(**kw)
        assert fn() == code, what
        _untouched(pr, W, what)
    for name in ("x", "params", "grads", "ws"):        # a pointer 4 bytes off 16-byte alignment
        fn, W, _ = pr.call()
        ptr = dict(x=pr.x.ptr, params=W["params"].ptr, grads=W["grads"].ptr, ws=W["ws"].ptr)[name]
        fn, W2, _ = pr.call(**{name: off(ptr)})
        assert fn() == EINVAL, name + " misaligned"
        _untouched(pr, W, name + " misaligned")
        _untouched(pr, W2, name + " misaligned")
    _, lib = _libs()
    assert lib.ltrx_fc_listnet_workspace_bytes(0, 16, 12, 16, 100) == 0 and lib.ltrx_fc_linear_listnet_workspace_bytes(0, 12) == 0


def _untouched(pr, W, what):
    torch.cuda.synchronize()
    for name in ("params", "scores", "dsc", "hid", "loss", "grads", "m", "v", "step"):
        W[name].unchanged("a refused call (%s) wrote %s" % (what, name))
    assert W["ws"].untouched(), "a refused call (%s) wrote its workspace" % what
    pr.x.unchanged(what)
    pr.y.unchanged(what)
