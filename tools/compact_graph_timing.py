"""FusedTrainer(compact="graph") against FusedTrainer(compact=True) on the same build, in one run (needs the MI355X).

    python tools/compact_graph_timing.py [--shapes shipped64,config3_64,config3_256] [--batches 64] [--steps 256] [--out FILE]

Per shape: two trainers from the same initial weights, ``--batches`` distinct ragged batches of bench.synth_batch (lognormal slate
lengths, about 47 % of the slots valid) with their host lengths, as a DeviceLoader hands them over.  Every batch is stepped three
times through both arms first, so every row bucket of the graph arm is warmed up and captured before anything is timed.  Then the
arms ALTERNATE: each timed window is ``--steps`` steps of one arm between two device synchronises, cycling through the batches, and
every arm gets two windows (graph, compact, graph, compact).  Reported per arm: ms per step and valid items per second of both
windows and their spread; for the graph arm the bucket histogram of one pass over the batches, the share of alignment rows (of both
arms: compact=True rounds up to 32 rows), captures and evictions.  Writes a markdown report (default profiles/compact_graph.md) and
prints one JSON line per shape."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from allrank_amd.engine import FusedTrainer  # noqa: E402

CONFIG3 = bench.WORKLOADS["attn_approxndcg"]
SHAPES = {
    # a shipped-config shape: small model, 64 slates per batch
    "shipped64": dict(w=dict(n_features=136, fc_sizes=[128], N=4, h=4, d_ff=512, loss="lambdaLoss",
                             loss_args=dict(weighing_scheme="ndcgLoss2PP_scheme")), B=64, L=240, dropout=0.1),
    "config3_64": dict(w=CONFIG3, B=64, L=240, dropout=0.0),
    "config3_256": dict(w=CONFIG3, B=256, L=240, dropout=0.0),
}


def run_shape(name, nb, steps, dev):
    s = SHAPES[name]
    w, B, L = s["w"], s["B"], s["L"]
    x, y, _ = bench.synth_batch(nb * B, L, w["n_features"], 4711, dev, ragged=True)
    lens = (y != -1).sum(1).to(torch.int32).cpu()
    batches = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B], lens[i * B:(i + 1) * B]) for i in range(nb)]
    counts = [int(b[2].sum()) for b in batches]
    arms = {}
    for arm, compact in (("graph", "graph"), ("compact", True)):
        model = bench.build_model(w, dev, s["dropout"])
        arms[arm] = FusedTrainer(model, w["loss"], w.get("loss_args") or {}, B, L, lr=1e-3, use_graph=True, compact=compact, seed=1)
    for _ in range(3):                                            # eager, eager, capture of every bucket (the compact arm: warm caches)
        for tr in arms.values():
            for xb, yb, hl in batches:
                tr.step(xb, yb, lengths=hl)
    torch.cuda.synchronize()
    g = arms["graph"]
    warm_modes = dict(g.mode_counts)
    hist = {}
    for r in g.bucket_of(counts):
        hist[r] = hist.get(r, 0) + 1
    windows = {arm: [] for arm in arms}
    for rep in range(2):
        for arm, tr in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                xb, yb, hl = batches[i % nb]
                tr.step(xb, yb, lengths=hl)
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
            items = sum(counts[i % nb] for i in range(steps))
            windows[arm].append(dict(ms_per_step=sec / steps * 1e3, valid_items_per_s=items / sec))
    timed_modes = {k: v - warm_modes.get(k, 0) for k, v in g.mode_counts.items()}
    rows_g, rows_c = g.bucket_of(counts), [max(32, (n + 31) // 32 * 32) for n in counts]
    rec = dict(shape=name, B=B, L=L, batches=nb, steps_per_window=steps, valid_fraction=sum(counts) / float(nb * B * L),
               windows=windows, buckets=dict(sorted(hist.items())),
               alignment_share=dict(graph=1.0 - sum(counts) / float(sum(rows_g)), compact=1.0 - sum(counts) / float(sum(rows_c))),
               captures=g.mode_counts["capture"], evictions=g._step_graphs.evictions, live_graphs=len(g._graphs),
               timed_modes=timed_modes, losses_finite=all(bool(torch.isfinite(t.loss.loss).all()) for t in arms.values()))
    del arms, g, batches, x, y
    torch.cuda.empty_cache()
    return rec


def report(recs):
    out = ["# compact=\"graph\" against compact=True\n",
           "Written by `tools/compact_graph_timing.py` (its docstring says how the windows are taken).  Both arms run in the same process",
           "on the same build and alternate; a window is a host clock around steps that end in a device synchronise.\n",
           "| shape | arm | ms / step (window 1, 2) | valid items / s (window 1, 2) | spread of ms / step |",
           "|---|---|---|---|---|"]
    for r in recs:
        for arm in ("graph", "compact"):
            a, b = r["windows"][arm]
            out.append("| %s (B %d, L %d) | %s | %.3f, %.3f | %.0f, %.0f | %.1f %% |"
                       % (r["shape"], r["B"], r["L"], arm, a["ms_per_step"], b["ms_per_step"], a["valid_items_per_s"], b["valid_items_per_s"],
                          100.0 * abs(a["ms_per_step"] - b["ms_per_step"]) / min(a["ms_per_step"], b["ms_per_step"])))
    out += ["", "| shape | graph / compact (ms per step, means of the two windows) | valid slots | alignment rows: graph, compact | "
            "buckets (rows: batches of one pass) | captures | evictions | timed steps by mode |", "|---|---|---|---|---|---|---|---|"]
    for r in recs:
        m = {arm: sum(v["ms_per_step"] for v in r["windows"][arm]) / 2 for arm in r["windows"]}
        out.append("| %s | %.3f / %.3f = %.3f | %.1f %% | %.2f %%, %.2f %% | %s | %d | %d | %s |"
                   % (r["shape"], m["graph"], m["compact"], m["graph"] / m["compact"], 100 * r["valid_fraction"],
                      100 * r["alignment_share"]["graph"], 100 * r["alignment_share"]["compact"],
                      ", ".join("%d: %d" % kv for kv in r["buckets"].items()), r["captures"], r["evictions"], r["timed_modes"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="shipped64,config3_64,config3_256")
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_graph.md"))
    args = ap.parse_args()
    if args.batches < 64 or args.steps < 200:
        print("note: fewer than 64 batches or 200 steps per window is a rehearsal, not a measurement", file=sys.stderr)
    dev = torch.device("cuda", 0)
    recs = []
    for name in args.shapes.split(","):
        recs.append(run_shape(name, args.batches, args.steps, dev))
        print(json.dumps(recs[-1]), flush=True)
        with open(args.out, "w") as fh:                           # (after every shape: a later shape that fails keeps the earlier ones)
            fh.write(report(recs))


if __name__ == "__main__":
    main()
