"""ltrx_mha_fwd (mode 1: the exact fp32 arm at head widths 65..128) against ltrx_mha_fwd_wide (mode 1), interleaved in one process.

Shapes: the shipped wide-head configs (96 / 1 and 144 / 2) at 64 x 240 and 256 x 240 padded slates, and the validation shape of
profiles/rank_slates.md packed (64 slates, the longest 1,251 items, lognormal lengths around 100: about 11 % of the padded slots valid).
Every round times `iters` calls of one arm, then of the other, between device events; the figure of an arm is the median over the
rounds, the spread is (max - min) / median.  Also prints the largest |O_wide - O_exact| of each shape.  Needs the MI355X.

usage: python tools/mha_wide_timing.py [--iters 50] [--rounds 7] [--json out.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mha_wide_timing: no GPU -- nothing is measured")
    lib, dev = LB.lib(), "cuda"
    rows = []
    for name, B, L, h, dk, packed in SHAPES:
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
        outs = {arm: (torch.zeros(n, d, device=dev), torch.zeros(B, h, L, device=dev)) for arm in ("exact", "wide")}
        st = LB.stream_of(qkv)

        def call(arm):
            fn = lib.ltrx_mha_fwd if arm == "exact" else lib.ltrx_mha_fwd_wide
            o, lse = outs[arm]
            LB.check(fn(LB.ptr(qkv), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d, LB.ptr(mask), B, L, h, dk, 3 * d, LB.ptr(o), d, LB.ptr(lse),
                        0.0, 0, None, LB.ptr(cu), LB.ptr(order), 1, st), arm)

        times = {"exact": [], "wide": []}
        for arm in times:
            for _ in range(5):
                call(arm)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for arm in times:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    call(arm)
                b.record()
                torch.cuda.synchronize()
                times[arm].append(a.elapsed_time(b) / args.iters * 1e3)
        med = {arm: statistics.median(t) for arm, t in times.items()}
        row = dict(shape=name, B=B, L=L, h=h, d_k=dk, rows=n, exact_us=med["exact"], wide_us=med["wide"], ratio=med["exact"] / med["wide"],
                   exact_spread=(max(times["exact"]) - min(times["exact"])) / med["exact"],
                   wide_spread=(max(times["wide"]) - min(times["wide"])) / med["wide"],
                   max_abs_o_diff=float((outs["wide"][0] - outs["exact"][0]).abs().max()))
        rows.append(row)
        print("%-20s h %d d_k %3d rows %6d   exact %8.1f us (spread %4.1f %%)   wide %8.1f us (spread %4.1f %%)   exact / wide %5.2f   max |dO| %.2e"
              % (name, h, dk, n, row["exact_us"], 100 * row["exact_spread"], row["wide_us"], 100 * row["wide_spread"], row["ratio"],
                 row["max_abs_o_diff"]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(dict(iters=args.iters, rounds=args.rounds, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
