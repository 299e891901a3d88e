"""Clicks on ranked slates: the device call, ``click_on_slates`` end to end and a host baseline, in one run (needs the MI355X).

    python tools/click_timing.py [--iters 20] [--reps 5] [--host-slates 16] [--out FILE]

Batches: "web" -- the WEB30K-validation-like batch of tools/rank_timing.py, 64 slates padded to 1,251 items, lognormal lengths around
100 (about 11 % of the slots valid), 136 features -- and "dense", 256 slates of 240 items.  Labels 0 .. 4 in WEB30K's proportions.
Click models: "shipped", Diverse(Cascade(eta 1, threshold 2), q 0.5) of scripts/local_config_click_model.json, and "all",
Diverse(OnlyRelevant(0), q 0.5): every item a candidate, the worst case for the greedy scan.

Arms, per batch and model:
  kernel          ltrx_click_slates_cu alone on tensors in device memory, margin_out NULL (the product's call: a slate with fewer than two
                  candidates skips its distance work);
  kernel+margins  the same call with margin_out given: every slate computes its distances and its quantile -- the difference to
                  `kernel` is the distance and selection work the skip saves, the difference between the models is the greedy scan;
  end_to_end      ``clicks.click_on_slates`` from CPU tensors: the draw, the uploads, the launch, the copy back, the Python filter;
  host            where scipy imports: the reference's algorithm per slate on the host in its cheapest form (ONE cdist per slate, np.quantile,
                  a greedy pass that looks distances up; the reference itself calls cdist again for every candidate), on
                  ``--host-slates`` slates of the batch, scaled to the batch by item pairs.  The reference is not on this machine.
A window is a host clock around ``--iters`` calls that end in a device synchronise, ``--reps`` windows per arm, arms alternating; the
median is reported with the spread.  Writes a markdown report (default profiles/click_slates.md) and prints one JSON line."""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from allrank_amd import _lib as LB, clicks as C  # noqa: E402

F = 136
with open(LB.HEADER_PATH) as _fh:
    _h = _fh.read()
LDS_LEN = int(re.search(r"#define LTRX_CLICK_LDS_SLATE_LEN (\d+)", _h).group(1))
SLABS = int(re.search(r"#define LTRX_CLICK_SLAB_WORKGROUPS (\d+)", _h).group(1))


def make_batch(kind):
    rng = np.random.default_rng(30)
    if kind == "web":
        B, L = 64, 1251
        lens = np.clip(np.round(rng.lognormal(np.log(100.0), 0.6, B)), 1, L).astype(np.int64)
        lens[0] = L
    else:
        B, L = 256, 240
        lens = np.full(B, L, dtype=np.int64)
    X = np.zeros((B, L, F), dtype=np.float32)
    y = np.full((B, L), -1.0, dtype=np.float32)
    for b, n in enumerate(lens):
        X[b, :n] = rng.standard_normal((n, F)).astype(np.float32)
        y[b, :n] = rng.choice(5, n, p=[0.52, 0.32, 0.13, 0.02, 0.01])
    return torch.tensor(X), torch.tensor(y), lens


def host_clicks(model, X, y, lens, slates):
    """the reference's algorithm on the host, cheapest form; seconds for ``slates`` and the item pairs they hold"""
    from scipy.spatial.distance import cdist
    t0 = time.perf_counter()
    pairs = 0
    for b in slates:
        n = int(lens[b])
        rows, lab = X[b, :n].numpy(), y[b, :n].numpy()
        d = cdist(rows, rows, metric="euclidean")
        margin = np.quantile(d[np.triu_indices(n, 1)], q=model.q_percentile) if n > 1 else 0.0
        cand = np.flatnonzero(model.inner.click((rows, lab)))
        kept = []
        for i in cand:
            if all(d[j, i] > margin for j in kept):
                kept.append(i)
        pairs += n * (n - 1) // 2
    return time.perf_counter() - t0, pairs


def windows(arms, iters, reps):
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-slates", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "click_slates.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "click_timing needs the MI355X"
    dev = torch.device("cuda", 0)
    lib, st = LB.lib(), LB.launch_stream(dev)
    models = {"shipped": C.Diverse(C.Cascade(1, 2), 0.5), "all": C.Diverse(C.OnlyRelevant(0), 0.5)}
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    rec = dict(F=F, iters=args.iters, reps=args.reps, scipy=have_scipy, batches={})
    rows = []
    for kind in ("web", "dense"):
        X, y, lens = make_batch(kind)
        B, L = y.shape
        xb, yb = X.to(dev), y.to(dev)
        cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device=dev)
        order = torch.tensor(np.argsort(-lens, kind="stable").astype(np.int32), device=dev)
        max_len = int(lens.max())
        out = torch.empty((B, L), dtype=torch.float32, device=dev)
        mg = torch.empty((B,), dtype=torch.float64, device=dev)
        ws = LB.workspace(lib.ltrx_click_workspace_bytes(B, max_len, 1), xb)
        u = torch.tensor(np.random.RandomState(1).rand(int(lens.sum())), device=dev)
        info = dict(B=int(B), L=int(L), items=int(lens.sum()), pairs=int((lens * (lens - 1) // 2).sum()),
                    valid_fraction=float(lens.sum()) / (B * L), ws_bytes=int(ws.numel()), ms={}, spread_pct={}, clicks={})
        for mname, model in models.items():
            plan, why = C.plan_of(model)
            assert plan is not None, why
            table = torch.tensor(1 / np.arange(1, L + 1) ** plan["eta"], dtype=torch.float64, device=dev) if plan["kind"] == "cascade" else None
            uu = u if plan["kind"] == "cascade" else None

            def kernel(margins, plan=plan, table=table, uu=uu):
                return lambda: C.click_slates_cu(lib, st, xb, yb, cu, order, B, max_len, out, plan, uu, table, mg if margins else None, ws)

            def end_to_end(model=model):
                np.random.seed(1)
                return C.click_on_slates((X, y), model, include_empty=True)

            arms = {"kernel": kernel(False), "kernel+margins": kernel(True), "end_to_end": end_to_end}
            for fn in arms.values():                                   # warm-up of every arm, and the two kernel forms agree
                fn()
            kernel(False)()
            a = out.clone()
            kernel(True)()
            torch.cuda.synchronize()
            assert torch.equal(a, out), "the skip path changed the clicks"
            assert C.last_run["engine"] == "device", C.last_run
            info["clicks"][mname] = int((out == 1).sum())
            t = windows(arms, args.iters, args.reps)
            for k, v in t.items():
                info["ms"]["%s.%s" % (mname, k)] = statistics.median(v) * 1e3
                info["spread_pct"]["%s.%s" % (mname, k)] = 100.0 * (max(v) - min(v)) / statistics.median(v)
            if have_scipy:
                pick = list(range(0, B, max(1, B // args.host_slates)))[:args.host_slates]
                host_clicks(model, X, y, lens, pick[-1:])              # warm-up (scipy's first call)
                np.random.seed(1)
                sec, pairs = host_clicks(model, X, y, lens, pick)
                info["ms"]["%s.host" % mname] = sec * 1e3 * info["pairs"] / max(pairs, 1)
                info["host_slates"] = len(pick)
        rec["batches"][kind] = info
        for mname in models:
            m, s = info["ms"], info["spread_pct"]
            rows.append("| %s | %s | %.3f (%.1f %%) | %.3f (%.1f %%) | %.2f (%.1f %%) | %s | %d |"
                        % (kind, mname, m[mname + ".kernel"], s[mname + ".kernel"], m[mname + ".kernel+margins"], s[mname + ".kernel+margins"],
                           m[mname + ".end_to_end"], s[mname + ".end_to_end"],
                           "%.0f" % m[mname + ".host"] if have_scipy else "not measured", info["clicks"][mname]))
    print(json.dumps(rec), flush=True)
    w, d = rec["batches"]["web"], rec["batches"]["dense"]
    text = ["# click_on_slates: ltrx_click_slates_cu against the per-slate host loop\n",
            "Written by `tools/click_timing.py` (its docstring says what the arms are and how the windows are taken).  One process, one build,",
            "the arms alternate; a window is a host clock around %d calls that end in a device synchronise; medians of %d windows, the spread"
            % (args.iters, args.reps),
            "of the windows in brackets.  %d features.  web: %d slates padded to %d, %.1f %% of the slots valid (%d items, %.2f M pairs); dense:"
            % (F, w["B"], w["L"], 100 * w["valid_fraction"], w["items"], w["pairs"] / 1e6),
            "%d slates of %d (%d items, %.2f M pairs).  Workspace of the call: web %.1f MB, dense %.1f MB.\n"
            % (d["B"], d["L"], d["items"], d["pairs"] / 1e6, w["ws_bytes"] / 1e6, d["ws_bytes"] / 1e6),
            "| batch | model | kernel, ms | kernel + margins, ms | click_on_slates end to end, ms | host loop, ms (scaled) | clicks |",
            "|---|---|---|---|---|---|---|"] + rows
    text += ["", "Kernel share of `click_on_slates` end to end (the rest is the draw, the uploads of X, y and the uniforms, the copy back and the",
             "Python filter): " + "; ".join("%s / %s %.0f %%" % (k, m, 100 * rec["batches"][k]["ms"][m + ".kernel"] / rec["batches"][k]["ms"][m + ".end_to_end"])
                                            for k in ("web", "dense") for m in models) + ".", ""]
    for k, b in (("web", w), ("dense", d)):
        n = b["L"]
        tiles = ((n + 63) // 64) * ((n + 63) // 64 + 1) // 2
        ops = 3.0 * tiles * 4096 * F
        per = (b["B"] + SLABS - 1) // SLABS if n > LDS_LEN else 1
        text.append("%s: the launch lasts as long as its slowest workgroup.  The longest slate has %d items = %d pairs, computed as %d tiles of 64 x 64"
                    % (k, n, n * (n - 1) // 2, tiles))
        text.append("pairs x %d features x 3 fp64 operations (subtract, multiply, add; no FMA by contract) = %.0f M operations on ONE CU; a workgroup"
                    % (F, ops / 1e6))
        text.append("walks up to %d such slate(s).  With every slate computing distances (`all`, or `kernel + margins`) the launch takes %.2f ms:"
                    % (per, b["ms"]["all.kernel"]))
        text.append("at least %.0f G fp64 operations / s on that CU.  The distance phase bounds the kernel: `all` (every item a candidate, the greedy"
                    % (per * ops / b["ms"]["all.kernel"] / 1e6))
        text.append("scan's worst case) costs %+.3f ms over `shipped` + margins (distances and selection for every slate, a short scan); the skip"
                    % (b["ms"]["all.kernel"] - b["ms"]["shipped.kernel+margins"]))
        text.append("of slates with fewer than two candidates saves %.3f ms of the shipped model's %.3f."
                    % (b["ms"]["shipped.kernel+margins"] - b["ms"]["shipped.kernel"], b["ms"]["shipped.kernel+margins"]))
        text.append("")
    text += ["The host column is the reference's ALGORITHM in its cheapest form (one scipy cdist per slate; the reference calls cdist again for",
             "every candidate), %s.  ONE pass, not repeated: its spread is not measured, read it as an order of magnitude.  The reference itself"
             % ("measured on %d slates of the batch and scaled by pairs" % w.get("host_slates", 0) if have_scipy else "not measured: scipy is missing"),
             "has not been run on this machine, and the share of an unmodified `rank_and_click` run that its two host loops take has not been",
             "measured."]
    with open(args.out, "w") as fh:
        fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
