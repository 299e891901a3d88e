"""The exact fp32 arm at head widths 65..128 (ltrx_mha_fwd / ltrx_mha_bwd, mode 1) against the opt-in split-bf16 kernels
(ltrx_mha_fwd_wide / ltrx_mha_bwd_wide, mode 1), interleaved in one process.

Shapes: the shipped wide-head configs (96 / 1 and 144 / 2) at 64 x 240 and 256 x 240 padded slates, and the validation shape of
profiles/rank_slates.md packed (64 slates, the longest 1,251 items, lognormal lengths around 100: about 11 % of the padded slots valid).
Every round times `iters` calls of one arm, then of the other, between device events; the figure of an arm is the median over the
rounds, the spread is (max - min) / median.  Also prints the largest difference between the arms' results on each shape.
  fwd:  the forward calls, p_drop 0.
  bwd:  the backward calls on the exact forward's o / lse, p_drop 0, and the first shape again at p_drop 0.1.
  step: one whole training step of fc[96] + 2 x (d 96, h 1, d_ff 384), listNet, 64 x 240, FusedTrainer(wide_heads=True) against
        FusedTrainer(wide_heads=True, wide_backward=True), captured steps, alternating the same way.
Needs the MI355X.

usage: python tools/mha_wide_timing.py [--what fwd,bwd,step] [--iters 50] [--rounds 7] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from allrank_amd import _lib as LB  # noqa: E402

SHAPES = [("64 x 240 padded", 64, 240, 1, 96, False), ("256 x 240 padded", 256, 240, 1, 96, False),
          ("64 x 240 padded", 64, 240, 2, 72, False), ("256 x 240 padded", 256, 240, 2, 72, False),
          ("64 x <=1251 packed", 64, 1251, 1, 96, True)]


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


def attention(what, shape, p_drop, args):
    lib, dev = LB.lib(), "cuda"
    name, B, L, h, dk, packed = shape
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
    outs = {arm: (torch.zeros(n, d, device=dev), torch.zeros(B, h, L, device=dev), torch.zeros(n, 3 * d, device=dev)) for arm in ("exact", "wide")}
    ws = torch.zeros(lib.ltrx_mha_bwd_workspace_bytes(B, L, h, dk, 1), dtype=torch.uint8, device=dev)
    st = LB.stream_of(qkv)
    q, k, v = LB.ptr(qkv), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d

    def fwd(arm, into):
        fn = lib.ltrx_mha_fwd if arm == "exact" else lib.ltrx_mha_fwd_wide
        LB.check(fn(q, k, v, LB.ptr(mask), B, L, h, dk, 3 * d, LB.ptr(outs[into][0]), d, LB.ptr(outs[into][1]), p_drop, 0, None, LB.ptr(cu),
                    LB.ptr(order), 1, st), arm)

    def bwd(arm):
        fn = lib.ltrx_mha_bwd if arm == "exact" else lib.ltrx_mha_bwd_wide
        o, lse, dqkv = outs[arm]
        LB.check(fn(q, k, v, LB.ptr(mask), LB.ptr(o), LB.ptr(do), LB.ptr(lse), B, L, h, dk, 3 * d, d, LB.ptr(dqkv), dqkv.data_ptr() + 4 * d,
                    dqkv.data_ptr() + 8 * d, 3 * d, p_drop, 0, None, LB.ptr(cu), LB.ptr(order), 1, LB.ptr(ws), st), arm)

    if what == "fwd":
        res = alternate(("exact", "wide"), lambda arm: fwd(arm, arm), args.iters, args.rounds)
        diff = float((outs["wide"][0] - outs["exact"][0]).abs().max())
    else:
        for arm in ("exact", "wide"):             # both backward arms run on the exact forward's o / lse
            fwd("exact", arm)
        res = alternate(("exact", "wide"), bwd, args.iters, args.rounds)
        diff = float((outs["wide"][2] - outs["exact"][2]).abs().max())
    row = dict(what=what, shape=name, B=B, L=L, h=h, d_k=dk, rows=n, p_drop=p_drop, exact_us=res["exact"][0], wide_us=res["wide"][0],
               ratio=res["exact"][0] / res["wide"][0], exact_spread=res["exact"][1], wide_spread=res["wide"][1], max_abs_diff=diff,
               gap_over_larger_spread=(res["exact"][0] - res["wide"][0]) / max(res["exact"][0] * res["exact"][1], res["wide"][0] * res["wide"][1]))
    print("%s %-20s h %d d_k %3d rows %6d p %.1f   exact %8.1f us (spread %4.1f %%)   wide %8.1f us (spread %4.1f %%)   exact / wide %5.2f   "
          "max |diff| %.2e" % (what, name, h, dk, n, p_drop, row["exact_us"], 100 * row["exact_spread"], row["wide_us"], 100 * row["wide_spread"],
                               row["ratio"], diff), flush=True)
    return row


def step(args):
    from allrank_amd.engine import FusedTrainer
    from allrank_amd.model import make_model
    B, L, F = 64, 240, 136
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(B, L, F, device="cuda", generator=g)
    y = torch.randint(0, 5, (B, L), device="cuda", generator=g).float()
    trainers = {}
    for arm, kw in (("exact backward", {}), ("wide backward", dict(wide_backward=True))):
        torch.manual_seed(42)
        model = make_model(dict(sizes=[96], input_norm=False, activation=None, dropout=0.0),
                           dict(N=2, d_ff=384, h=1, positional_encoding=None, dropout=0.0), dict(d_output=1, output_activation=None), F).to("cuda")
        trainers[arm] = FusedTrainer(model, "listNet", {}, B, L, lr=1e-3, use_graph=True, wide_heads=True, **kw)
    assert trainers["wide backward"].attention_backward == "wide" and trainers["exact backward"].attention_backward == "default"
    res = alternate(tuple(trainers), lambda arm: trainers[arm].step(x, y), args.iters, args.rounds)
    row = dict(what="step", model="fc[96] + 2 x (d 96, h 1, d_ff 384), listNet", B=B, L=L,
               **{arm.replace(" ", "_") + "_us": res[arm][0] for arm in res}, **{arm.replace(" ", "_") + "_spread": res[arm][1] for arm in res})
    print("step 64 x 240: " + "   ".join("%s %8.1f us (spread %4.1f %%)" % (arm, res[arm][0], 100 * res[arm][1]) for arm in res), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="fwd,bwd,step")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mha_wide_timing: no GPU -- nothing is measured")
    rows = []
    for what in args.what.split(","):
        if what == "step":
            rows.append(step(args))
        else:
            rows += [attention(what, shape, 0.0, args) for shape in SHAPES]
            if what == "bwd":
                rows.append(attention(what, SHAPES[0], 0.1, args))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(dict(iters=args.iters, rounds=args.rounds, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
