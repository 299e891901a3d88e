"""ltrx_mha_fwd (mode 1: the exact fp32 arm at head widths up to 32) against ltrx_mha_fwd_narrow (mode 1), interleaved in one process.

Shapes: 64 x 240 and 256 x 240 padded slates at h 4 / d_k 32 (a 128 / 4 transformer) and h 4 / d_k 16, with p_drop 0 and 0.3, and the
validation shape of profiles/mha_wide.md packed (64 slates, the longest 1,251 items, lognormal lengths around 100: about 11 % of the
padded slots valid).  Every round times `iters` calls of one arm, then of the next, between device events; the figure of an arm is the
median over the rounds, the spread is (max - min) / median.  Also prints the largest |O_narrow - O_exact| of each shape.
--alt-lib PATH adds a third arm: ltrx_mha_fwd_narrow of a second build of the library (how the one-against-two query blocks per
wave choice was timed: the other build held two 32-query blocks per wave).
--step adds one captured training step and one ``score()`` pass of fc[128] + 4 x (d 128, h 4, d_ff 512), dropout 0.3, listNet, at
64 x 240: FusedTrainer() against FusedTrainer(narrow_heads=True).
--backward times the backward instead, on the same shapes: ltrx_mha_bwd (mode 1: the exact arm) against ltrx_mha_bwd_narrow; with
--step, FusedTrainer(narrow_heads=True) against FusedTrainer(narrow_heads="both").  Needs the MI355X.

usage: python tools/mha_narrow_timing.py [--iters 50] [--rounds 7] [--alt-lib libltrx_other.so] [--backward] [--step] [--json out.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from allrank_amd import _lib as LB  # noqa: E402

SHAPES = [(name, B, 240, 4, dk, False, p) for dk in (32, 16) for name, B in (("64 x 240 padded", 64), ("256 x 240 padded", 256))
          for p in (0.0, 0.3)]
SHAPES += [("64 x <=1251 packed", 64, 1251, 4, 32, True, 0.0)]


def alternate(arms, call, iters, rounds):
    """{arm: (median us per call, spread)}: 5 warm-up calls per arm, then `rounds` rounds of one `iters`-call window per arm"""
    times = {arm: [] for arm in arms}
    for arm in arms:
        for _ in range(5):
            call(arm)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for arm in arms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                call(arm)
            b.record()
            torch.cuda.synchronize()
            times[arm].append(a.elapsed_time(b) / iters * 1e3)
    return {arm: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for arm, t in times.items()}


def _row(res, **head):
    row = dict(head)
    for arm, (us, spread) in res.items():
        row[arm + "_us"], row[arm + "_spread"] = us, spread
    return row, "  ".join("%s %8.1f us (spread %4.1f %%)" % (arm, us, 100 * spread) for arm, (us, spread) in res.items())


def attention(shape, fns, args):
    dev = "cuda"
    name, B, L, h, dk, packed, p = shape
    d = h * dk
    g = torch.Generator(device=dev).manual_seed(5)
    if packed:
        lens = np.clip(np.round(np.random.default_rng(3).lognormal(np.log(100.0), 0.6, B)), 1, L).astype(np.int64)
        lens[0] = L
        n = int(lens.sum())
        cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
        order = torch.tensor(np.argsort(-lens, kind="stable"), dtype=torch.int32, device=dev)
        mask = None
    else:
        n, cu, order = B * L, None, None
        mask = torch.zeros((B, L), dtype=torch.uint8, device=dev)
    qkv = torch.randn(n, 3 * d, device=dev, generator=g)
    outs = {arm: (torch.zeros(n, d, device=dev), torch.zeros(B, h, L, device=dev)) for arm in fns}
    st = LB.stream_of(qkv)

    def call(arm):
        o, lse = outs[arm]
        LB.check(fns[arm](LB.ptr(qkv), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d, LB.ptr(mask), B, L, h, dk, 3 * d, LB.ptr(o), d,
                          LB.ptr(lse), p, 7, None, LB.ptr(cu), LB.ptr(order), 1, st), arm)

    res = alternate(tuple(fns), call, args.iters, args.rounds)
    row, text = _row(res, what="fwd", shape=name, B=B, L=L, h=h, d_k=dk, p_drop=p, rows=n, ratio=res["exact"][0] / res["narrow"][0],
                     max_abs_o_diff=float((outs["narrow"][0] - outs["exact"][0]).abs().max()))
    print("%-20s h %d d_k %2d p %.1f rows %6d  %s   exact / narrow %5.2f   max |dO| %.2e"
          % (name, h, dk, p, n, text, row["ratio"], row["max_abs_o_diff"]), flush=True)
    return row


def attention_backward(shape, lib, args):
    """`attention` for the backward: ltrx_mha_bwd (mode 1: the exact arm) against ltrx_mha_bwd_narrow on the o / lse of one
    ltrx_mha_fwd_narrow call; also the largest |dQ, dK, dV difference| between the arms"""
    dev = "cuda"
    name, B, L, h, dk, packed, p = shape
    d = h * dk
    g = torch.Generator(device=dev).manual_seed(5)
    if packed:
        lens = np.clip(np.round(np.random.default_rng(3).lognormal(np.log(100.0), 0.6, B)), 1, L).astype(np.int64)
        lens[0] = L
        n = int(lens.sum())
        cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
        order = torch.tensor(np.argsort(-lens, kind="stable"), dtype=torch.int32, device=dev)
        mask = None
    else:
        n, cu, order = B * L, None, None
        mask = torch.zeros((B, L), dtype=torch.uint8, device=dev)
    qkv = torch.randn(n, 3 * d, device=dev, generator=g)
    do = torch.randn(n, d, device=dev, generator=g)
    o, lse = torch.zeros(n, d, device=dev), torch.zeros(B, h, L, device=dev)
    ws = torch.zeros(lib.ltrx_mha_bwd_workspace_bytes(B, L, h, dk, 1), dtype=torch.uint8, device=dev)
    fns = {"exact": lib.ltrx_mha_bwd, "narrow": lib.ltrx_mha_bwd_narrow}
    outs = {arm: torch.zeros(n, 3 * d, device=dev) for arm in fns}
    st = LB.stream_of(qkv)
    q, k, v = LB.ptr(qkv), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d
    LB.check(lib.ltrx_mha_fwd_narrow(q, k, v, LB.ptr(mask), B, L, h, dk, 3 * d, LB.ptr(o), d, LB.ptr(lse), p, 7, None, LB.ptr(cu), LB.ptr(order),
                                     1, st), "fwd_narrow")

    def call(arm):
        dx = outs[arm]
        LB.check(fns[arm](q, k, v, LB.ptr(mask), LB.ptr(o), LB.ptr(do), LB.ptr(lse), B, L, h, dk, 3 * d, d, LB.ptr(dx), dx.data_ptr() + 4 * d,
                          dx.data_ptr() + 8 * d, 3 * d, p, 7, None, LB.ptr(cu), LB.ptr(order), 1, LB.ptr(ws), st), arm)

    res = alternate(tuple(fns), call, args.iters, args.rounds)
    row, text = _row(res, what="bwd", shape=name, B=B, L=L, h=h, d_k=dk, p_drop=p, rows=n, ratio=res["exact"][0] / res["narrow"][0],
                     max_abs_grad_diff=float((outs["narrow"] - outs["exact"]).abs().max()), max_abs_grad=float(outs["exact"].abs().max()))
    print("bwd %-20s h %d d_k %2d p %.1f rows %6d  %s   exact / narrow %5.2f   max |d grad| %.2e of %.2e"
          % (name, h, dk, p, n, text, row["ratio"], row["max_abs_grad_diff"], row["max_abs_grad"]), flush=True)
    return row


def step(args, arms=(("default", {}), ("narrow", dict(narrow_heads=True)))):
    from allrank_amd.engine import FusedTrainer
    from allrank_amd.model import make_model
    B, L, F = 64, 240, 136
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(B, L, F, device="cuda", generator=g)
    y = torch.randint(0, 5, (B, L), device="cuda", generator=g).float()
    trainers = {}
    for arm, kw in arms:
        torch.manual_seed(42)
        model = make_model(dict(sizes=[128], input_norm=False, activation=None, dropout=0.0),
                           dict(N=4, d_ff=512, h=4, positional_encoding=None, dropout=0.3), dict(d_output=1, output_activation=None), F).to("cuda")
        trainers[arm] = FusedTrainer(model, "listNet", {}, B, L, lr=1e-3, use_graph=True, **kw)
    for arm, kw in arms:
        assert trainers[arm].attention_forward == ("narrow" if kw else "default")
        assert trainers[arm].attention_backward == ("narrow" if kw.get("narrow_heads") == "both" else "default")
    rows = []
    for what, call in (("step", lambda arm: trainers[arm].step(x, y)), ("score", lambda arm: trainers[arm].score(x, y))):
        row, text = _row(alternate(tuple(trainers), call, args.iters, args.rounds), what=what,
                         model="fc[128] + 4 x (d 128, h 4, d_ff 512), p 0.3, listNet", B=B, L=L)
        rows.append(row)
        print("%s 64 x 240: %s" % (what, text), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--backward", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mha_narrow_timing: no GPU -- nothing is measured")
    lib = LB.lib()
    fns = {"exact": lib.ltrx_mha_fwd, "narrow": lib.ltrx_mha_fwd_narrow}
    if args.alt_lib:
        alt = ctypes.CDLL(os.path.abspath(args.alt_lib)).ltrx_mha_fwd_narrow
        alt.restype, alt.argtypes = LB.SIGNATURES["ltrx_mha_fwd_narrow"]
        fns["alt"] = alt
    if args.backward:
        rows = [attention_backward(shape, lib, args) for shape in SHAPES]
        if args.step:
            rows += step(args, (("narrow", dict(narrow_heads=True)), ("both", dict(narrow_heads="both"))))
    else:
        rows = [attention(shape, fns, args) for shape in SHAPES]
        if args.step:
            rows += step(args)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(dict(iters=args.iters, rounds=args.rounds, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
