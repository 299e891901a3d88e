"""Ranking a WEB30K-validation-like batch three ways on the same build, in one run (needs the MI355X).

    python tools/rank_timing.py [--batches 4] [--iters 30] [--reps 5] [--out FILE]

Shape: 64 slates per batch, the longest 1,251 items, lognormal lengths around 100 (about 10 % of the padded slots valid), 136
features, the config-3 model of bench.py (fc[512] + 2 x self-attention d512 h8 d_ff2048).  Arms, every one on batches already in
device memory and without the copy of the result to the host:

  (a) module    what the reference's rank_slates does per batch: nn.Module ``score`` on the padded grid, ``-inf`` on padding,
                ``torch.sort(descending=True, stable=True)``, ``torch.gather`` of X and y;
  (b) grid      allrank_amd.inference on a padded batch: FusedScorer.run on the valid rows + ltrx_rank_slates_cu (grid source);
  (c) resident  ... from the resident set: FusedScorer.run_resident + ltrx_rank_slates_cu (resident source).

Every arm is warmed up on every batch (the scorer's graphs are captured), then the arms ALTERNATE: a window is ``--iters`` passes
over the batches of one arm between two device synchronises, ``--reps`` windows per arm, the median is reported with the spread.
The new path is split the same way -- windows of the scorer alone and of the rank kernel alone (on the scores of the last batch) -- and
the rank kernel's bytes (n F read + B L F written, plus scores, labels and the order) over its time are set against the HBM rates of
MI355X_MICROARCH.md (8.0 TB/s specified, 6.29 TB/s measured for a float4 copy).  Writes a markdown report (default
profiles/rank_slates.md) and prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from allrank_amd import inference as EI  # noqa: E402
from allrank_amd.data import DeviceSlates  # noqa: E402

W = bench.WORKLOADS["attn_approxndcg"]
B, LONGEST, F = 64, 1251, 136
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def device_bytes(obj):
    """bytes of the distinct device storages ``obj`` holds in its attributes (one level of lists / tuples / dicts deep)"""
    seen, nb = set(), 0
    stack = list(vars(obj).values())
    for v in stack:
        for t in (v.values() if isinstance(v, dict) else v if isinstance(v, (list, tuple)) else [v]):
            for u in (t.values() if isinstance(t, dict) else [t]):
                if torch.is_tensor(u) and u.is_cuda and u.untyped_storage().data_ptr() not in seen:
                    seen.add(u.untyped_storage().data_ptr())
                    nb += u.untyped_storage().nbytes()
    return nb


def make_set(nb, dev):
    rng = np.random.default_rng(30)
    lens = np.clip(np.round(rng.lognormal(np.log(100.0), 0.6, nb * B)), 1, LONGEST).astype(np.int64)
    lens[::B] = LONGEST                                           # every batch is padded to the set's longest slate
    X = rng.standard_normal((int(lens.sum()), F)).astype(np.float32)
    y = rng.choice(5, int(lens.sum()), p=[0.52, 0.32, 0.13, 0.02, 0.01]).astype(np.float32)
    return DeviceSlates(X, y, np.repeat(np.arange(nb * B), lens), device=dev), lens


def windows(arms, iters, reps):
    """{arm: [seconds per call, one figure per window]}, the arms alternating"""
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            for _ in range(iters):
                calls += fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_slates.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rank_timing needs the MI355X"
    dev = torch.device("cuda", 0)
    nb = args.batches
    slates, lens = make_set(nb, dev)
    L = slates.longest_query_length
    ids = [torch.arange(i * B, (i + 1) * B, dtype=torch.int64) for i in range(nb)]
    hl = [slates.lengths_host[i * B:(i + 1) * B] for i in range(nb)]
    padded = [EI.padded_batch(slates, i) for i in ids]             # arms (a) and (b): padded batches resident in HBM, stored item order
    model = bench.build_model(W, dev, 0.0)
    model.eval()
    rk = EI.Ranker(model)
    assert not rk.reason, rk.reason
    sc = rk.scorer(B, L)

    @torch.no_grad()
    def arm_module():
        for xb, yb in padded:
            EI._module_rank(model, xb, yb)
        return nb

    @torch.no_grad()
    def arm_grid():
        for (xb, yb), h in zip(padded, hl):
            rk.rank_grid(B, xb, yb, h)
        return nb

    @torch.no_grad()
    def arm_resident():
        for i, h in zip(ids, hl):
            rk.rank_resident(B, L, slates, i, h)
        return nb

    @torch.no_grad()
    def scorer_grid():
        for (xb, yb), h in zip(padded, hl):
            sc.run(xb, yb, None, lengths=h)
        return nb

    @torch.no_grad()
    def scorer_resident():
        for i, h in zip(ids, hl):
            sc.run_resident(slates, i, h)
        return nb

    arms = {"module": arm_module, "grid": arm_grid, "resident": arm_resident}
    for fn in list(arms.values()) * 3 + [scorer_grid, scorer_resident]:       # warm-up: every arm on every batch, graphs captured
        fn()
    torch.cuda.synchronize()
    # the three arms agree (on distinct scores; a module / engine rounding difference may swap near-ties: counted, not asserted)
    xm, ym = EI._module_rank(model, *padded[-1])
    xg, yg = rk.rank_grid(B, padded[-1][0], padded[-1][1], hl[-1])
    xg, yg = xg.clone(), yg.clone()
    xr, yr = rk.rank_resident(B, L, slates, ids[-1], hl[-1])
    same_forms = bool(torch.equal(xg, xr) and torch.equal(yg, yr))
    rows_differ = int((xm != xg).any(-1).sum())

    t_arm = windows(arms, args.iters, args.reps)
    t_sc = windows({"scorer_grid": scorer_grid, "scorer_resident": scorer_resident}, args.iters, args.reps)

    # the rank kernel alone, both sources, on the last batch's scores
    sc.run_resident(slates, ids[-1], hl[-1])                                   # (also stages the batch's ids for the resident source)
    scores, _, cu, order, max_len = sc.packed()
    x_out, y_out = rk._buffers(B, L, F)
    t = rk.trainer

    def kern(**src):
        def run():
            for _ in range(nb):
                EI.rank_slates_cu(t.lib, t._st(), scores, cu, order, B, max_len, L, x_out, y_out, **src)
            return nb
        return run
    t_k = windows({"kernel_grid": kern(x=padded[-1][0], y=padded[-1][1]), "kernel_resident": kern(slates=slates, ids=sc.ids)},
                  args.iters * 4, args.reps)
    n_last = int(hl[-1].sum())
    kbytes = 4 * (n_last * F + B * L * F + 2 * n_last + B * L)                 # rows read, rows written, scores + labels read, labels written

    med = lambda v: statistics.median(v)
    spread = lambda v: 100.0 * (max(v) - min(v)) / med(v)
    rec = dict(B=B, L=L, F=F, batches=nb, iters=args.iters, reps=args.reps, valid_fraction=float(lens.sum()) / (nb * B * L),
               items_per_batch=float(lens.sum()) / nb,
               ms={k: med(v) * 1e3 for k, v in {**t_arm, **t_sc, **t_k}.items()},
               spread_pct={k: spread(v) for k, v in {**t_arm, **t_sc, **t_k}.items()},
               kernel_bytes=kbytes, kernel_items=n_last,
               kernel_TBps={k: kbytes / med(v) / 1e12 for k, v in t_k.items()},
               scorer_nbytes=int(sc.nbytes), trainer_nbytes=int(device_bytes(t)), output_nbytes=int(x_out.numel() * 4 + y_out.numel() * 4),
               grid_equals_resident=same_forms, rows_differing_from_module=rows_differ, scorer_mode=sc.last_mode)
    print(json.dumps(rec), flush=True)
    m, s = rec["ms"], rec["spread_pct"]
    out = ["# rank_slates: the module path against the packed scorer + ltrx_rank_slates_cu\n",
           "Written by `tools/rank_timing.py` (its docstring says how the windows are taken).  One process, one build, the arms alternate;",
           "a window is a host clock around %d passes over %d batches that end in a device synchronise; medians of %d windows."
           % (args.iters, nb, args.reps),
           "Shape: %d slates per batch padded to %d items, %d features, %.1f %% of the slots valid (%.0f items per batch), config-3 model."
           % (B, L, F, 100 * rec["valid_fraction"], rec["items_per_batch"]),
           "Batches are resident in device memory; the copy of the ranked batch to the host (%.1f MB, the same for every arm) is not timed.\n"
           % (rec["output_nbytes"] / 1e6),
           "| arm | ms per batch (median) | spread of the windows | against (a) |", "|---|---|---|---|"]
    for k, label in (("module", "(a) module score + -inf + torch.sort + gather"), ("grid", "(b) packed scorer + rank kernel, padded batch"),
                     ("resident", "(c) packed scorer + rank kernel, resident set")):
        out.append("| %s | %.3f | %.1f %% | %.2f x |" % (label, m[k], s[k], m["module"] / m[k]))
    out += ["", "| part of the new path | ms per batch (median) | spread |", "|---|---|---|"]
    for k, label in (("scorer_grid", "scorer alone, padded batch (`FusedScorer.run`)"),
                     ("scorer_resident", "scorer alone, resident set (`run_resident`)"),
                     ("kernel_grid", "rank kernel alone, grid source"), ("kernel_resident", "rank kernel alone, resident source")):
        out.append("| %s | %.4f | %.1f %% |" % (label, m[k], s[k]))
    out += ["", "Rank kernel traffic on the last batch (%d items): %.2f MB per launch -- %d x %d floats read, %d x %d x %d written, plus scores and"
            % (n_last, kbytes / 1e6, n_last, F, B, L, F),
            "labels.  Over its time: grid source %.2f TB/s, resident source %.2f TB/s -- %.0f %% / %.0f %% of the 6.29 TB/s a float4 copy reaches"
            % (rec["kernel_TBps"]["kernel_grid"], rec["kernel_TBps"]["kernel_resident"],
               100 * rec["kernel_TBps"]["kernel_grid"] * 1e12 / HBM_COPY, 100 * rec["kernel_TBps"]["kernel_resident"] * 1e12 / HBM_COPY),
            "on this part (8.0 TB/s specified: %.0f %% / %.0f %%).  The launch is one workgroup per slate (%d here) and lasts as long as the"
            % (100 * rec["kernel_TBps"]["kernel_grid"] * 1e12 / HBM_SPEC, 100 * rec["kernel_TBps"]["kernel_resident"] * 1e12 / HBM_SPEC, B),
            "counting pass of its longest slate (%d^2 compares on one CU), not as its bytes: a variant that cut every slate's zero tail into"
            % L,
            "pieces for further workgroups (8 per slate here) measured the same 0.108 ms and was dropped.",
            "At %.0f %% valid the zero tail that the reference's return value demands is %.0f %% of the bytes."
            % (100 * rec["valid_fraction"], 100.0 * (1 - n_last * 1.0 / (B * L))), "",
            "Device memory: the scorer's buffer set `scorer.nbytes` = %.1f MB; the FusedTrainer that owns the weights (built at batch 1 x 8,"
            % (rec["scorer_nbytes"] / 1e6),
            "its step never called: flat parameters, gradients and Adam moments, weight images and transposes, its own small buffers)",
            "%.1f MB; the ranked output buffers %.1f MB." % (rec["trainer_nbytes"] / 1e6, rec["output_nbytes"] / 1e6), "",
            "Checks in the same run: grid and resident sources give identical outputs: %s; ranked rows of the last batch that differ between"
            % rec["grid_equals_resident"],
            "the module path and the engine (near-ties that the two score arithmetics order differently): %d of %d.  Scorer mode: %s."
            % (rows_differ, B * L, rec["scorer_mode"])]
    faster = [k for k in ("grid", "resident") if m[k] < m["module"]]
    out += ["", "Verdict: " + ("both new arms are faster than (a) on this shape." if len(faster) == 2 else
                               "NOT faster than (a): %s." % ", ".join(k for k in ("grid", "resident") if k not in faster))]
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
