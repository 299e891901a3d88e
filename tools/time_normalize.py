"""Time the on-device feature normalisation (allrank_amd/normalize.py) on a synthetic resident set of MSLR-WEB30K fold size and write
profiles/feature_normalize.md.

    python tools/time_normalize.py [--out profiles/feature_normalize.md] [--runs 15] [--scale 1.0]

Data: train 2.27 M x 136, test and vali 0.75 M x 136 fp32, drawn on the device from a seed (counts and quarters; the columns of the
settings file's negative list hold values <= 0).  Settings: tests/golden/normalize_web30k.json (the reference script's defaults).

What is timed, each with a pair of device events around the calls on torch's current stream, after 3 warm-up rounds, as the median of
``--runs`` rounds (the spread = (max - min) / median of the rounds is printed beside it):
  * the three kernels' calls on the train role alone: ``minimum`` (one pass: 4 n F bytes read), the moments (two passes: 8 n F bytes
    read), ``apply`` (one pass: 4 n F read + 4 n F written);
  * ``fit`` over the three roles (three minima, one host read of 3 x 136 floats for the sign decision, the moments of train) and
    ``apply`` on the three roles;
  * for comparison a device-to-device copy of the same arrays (``Tensor.copy_`` between two contiguous device tensors: one
    hipMemcpyAsync; 4 n F read + 4 n F written).
The arms alternate inside a round.  ``apply`` works in place, so every round first restores the arrays from a pristine copy, outside the
timed windows.  GB/s = the bytes above over the median time; "of copy" = that rate over the copy's rate on the same arrays.

The reference's host script (parse three text files with scikit-learn, a numpy loop over the columns, dump three text files) has NOT
been timed in this project; no ratio to it is stated.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from allrank_amd.normalize import FeatureNormalizer  # noqa: E402

ROWS = {"train": 2270000, "test": 750000, "vali": 750000}
F = 136


class _Resident(object):
    """what FeatureNormalizer needs of a DeviceSlates: the item array"""

    def __init__(self, x):
        self.x_items = x


def make_role(n, nz, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.randint(0, 400, (n, F), device=dev, generator=g).float() / 4.0
    neg = [i for i in nz.features_negative if i < F]
    x[:, neg] = -x[:, neg]
    return x


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_normalize.md"))
    ap.add_argument("--settings", default=os.path.join(ROOT, "tests", "golden", "normalize_web30k.json"))
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--scale", type=float, default=1.0, help="row counts x this (rehearsals)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_normalize.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    nz = FeatureNormalizer.from_settings(args.settings)
    rows = {r: max(1, int(n * args.scale)) for r, n in ROWS.items()}
    pristine = {r: make_role(n, nz, 11 + k, dev) for k, (r, n) in enumerate(rows.items())}
    work = {r: x.clone() for r, x in pristine.items()}
    spare = {r: torch.empty_like(x) for r, x in pristine.items()}
    nbytes = {r: 4 * x.numel() for r, x in pristine.items()}
    total = sum(nbytes.values())

    def restore():
        for r in work:
            work[r].copy_(pristine[r])

    def fit():
        nz.fit(_Resident(work["train"]), others=(_Resident(work["test"]), _Resident(work["vali"])), roles=list(work))

    def apply(roles):
        for r in roles:
            nz.apply(_Resident(work[r]))

    def moments():
        nz.fit_with_minima(work["train"], [], ["train"])

    arms = {
        "minimum, train": (lambda: nz.minimum(work["train"]), nbytes["train"]),
        "moments, train (two passes)": (moments, 2 * nbytes["train"]),
        "apply, train": (lambda: apply(["train"]), 2 * nbytes["train"]),
        "copy, train": (lambda: spare["train"].copy_(work["train"]), 2 * nbytes["train"]),
        "fit, three roles": (fit, total + 2 * nbytes["train"]),
        "apply, three roles": (lambda: apply(list(work)), 2 * total),
        "copy, three roles": (lambda: [spare[r].copy_(work[r]) for r in work], 2 * total),
    }
    order = ["minimum, train", "moments, train (two passes)", "copy, train", "fit, three roles", "copy, three roles", "apply, train"]
    times = {k: [] for k in arms}
    for rnd in range(3 + args.runs):
        restore()
        torch.cuda.synchronize()
        got = {k: timed(arms[k][0]) for k in order}
        restore()                                       # apply, three roles: on pristine arrays again (fit above left the statistics)
        torch.cuda.synchronize()
        got["apply, three roles"] = timed(arms["apply, three roles"][0])
        if rnd >= 3:
            for k, v in got.items():
                times[k].append(v)
    report = nz.report
    med = {k: statistics.median(v) for k, v in times.items()}
    rate = {k: arms[k][1] / (med[k] * 1e-3) / 1e9 for k in arms}
    copy_of = lambda k: "copy, train" if k.endswith("train") or "train " in k else "copy, three roles"  # noqa: E731
    lines = ["# Feature normalisation on the device: fit and apply against a device-to-device copy",
             "",
             "Written by `tools/time_normalize.py` (its docstring says what the arms are and how the windows are taken).  %s, ROCm torch %s."
             % (torch.cuda.get_device_name(0), torch.__version__),
             "Synthetic resident set: train %d, test %d, vali %d rows x %d fp32 features (%.2f GB in all, train %.2f GB); settings: the"
             % (rows["train"], rows["test"], rows["vali"], F, total / 1e9, nbytes["train"] / 1e9),
             "reference script's defaults, %d of %d columns take the logarithm.  Device events, 3 warm-up rounds, medians of %d rounds, the"
             % (report["log"], F, args.runs),
             "spread of the rounds in brackets.",
             "",
             "| arm | bytes moved, GB | time, ms | GB/s | of the copy's GB/s |",
             "|---|---|---|---|---|"]
    for k in arms:
        spread = (max(times[k]) - min(times[k])) / med[k]
        lines.append("| %s | %.2f | %.3f (%.1f %%) | %.0f | %s |" % (k, arms[k][1] / 1e9, med[k], 100 * spread, rate[k],
                                                                   "1" if k.startswith("copy") else "%.2f" % (rate[k] / rate[copy_of(k)])))
    lines += ["",
              "`fit` = three minima (one pass per role), one host read of the minima, the two-pass moments of train; its time includes that",
              "host round trip.  The passes that evaluate t (moments, apply) take one fp64 logarithm per element of a log column",
              "and, in apply, one fp64 division per element; `minimum` (no fp64 arithmetic beyond the widening) shows what the access",
              "pattern alone reaches.  Whether the vector unit bounds the other passes has not been checked with counters.",
              "",
              "The reference's host script (scikit-learn parse of three text files, a numpy loop over the columns, three text dumps) has not",
              "been timed in this project: no ratio to it is stated here.", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
