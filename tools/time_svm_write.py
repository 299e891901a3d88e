"""Time the libsvm writer (allrank_amd/saving.py, allrank_amd/csrc/ltrx_svmwrite.hip) and write profiles/svm_write.md.

    python tools/time_svm_write.py [--out profiles/svm_write.md] [--runs 20] [--dir /tmp] [--scale 1.0]

Two chunks of fp32 standard normals, F = 136, drawn from a seed:
  * "web30k-vali": 64 slates x 1,251 slots of which the first 11 % are valid (labels 0 .. 4, -1 on padding) -- one validation batch of
    rank_and_click.py on MSLR-WEB30K;
  * "dense": 256 MiB of features (CHUNK_BYTES), every row valid, in slates of 1,251 rows -- one full chunk of the writer.
What is timed, after 3 warm-up rounds, as the median of ``--runs`` rounds (the spread = (max - min) / median beside it):
  * pass A (``ltrx_libsvm_line_bytes``) and pass B (``ltrx_libsvm_format``), each between a pair of device events on torch's current
    stream; GB/s = the OUTPUT bytes (the text) over the median time, for both passes (pass A writes 8 bytes per row; it is rated by the
    text it measures so that the two passes compare);
  * a device-to-device copy of as many bytes as the text has (``Tensor.copy_`` between two device tensors): the roof for a kernel whose
    output is that text;
  * ``write_to_libsvm_without_masked`` end to end from CPU tensors -- upload, both passes, the copy to pinned memory, the file -- on a
    host clock around the call (it ends with the file renamed, after the last device synchronisation); the target file system is named;
  * scikit-learn's ``dump_svmlight_file`` (a library, not the reference) on the first 20,000 kept rows of the same arrays, on the same
    host, 3 runs; the full-size figure beside it is SCALED from that sample by the row count, not measured.  Where scikit-learn does not
    import, the table says so.
The arms alternate inside a round.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from allrank_amd import _lib as LB, saving as S  # noqa: E402

F, L = 136, 1251
SAMPLE_ROWS = 20000


def make_chunk(name, scale, seed):
    """(x [N, L, F] fp32, y [N, L] fp32) on the host"""
    g = torch.Generator().manual_seed(seed)
    if name == "web30k-vali":
        n, valid = max(1, int(64 * scale)), int(round(0.11 * L))
    else:
        n, valid = max(1, int((S.CHUNK_BYTES // (L * F * 4)) * scale)), L
    x = torch.randn((n, L, F), generator=g)
    y = torch.randint(0, 5, (n, L), generator=g).float()
    x[:, valid:], y[:, valid:] = 0.0, -1.0
    return x, y


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def file_system_of(path):
    best = ("", "unknown")
    try:
        with open("/proc/mounts") as fh:
            for line in fh:
                _, mount, kind = line.split()[:3]
                if os.path.realpath(path).startswith(mount.rstrip("/") + "/") or mount == "/":
                    if len(mount) >= len(best[0]):
                        best = (mount, kind)
    except OSError:
        pass
    return "%s (mounted at %s)" % (best[1], best[0] or "?")


def sklearn_seconds(x, y, where):
    """median seconds of dump_svmlight_file on the first SAMPLE_ROWS kept rows, the rows it wrote; None where scikit-learn is absent"""
    try:
        from sklearn.datasets import dump_svmlight_file
    except ImportError:
        return None, 0
    keep = (y.reshape(-1) != -1).numpy()
    xs, ys = x.reshape(-1, F).numpy()[keep][:SAMPLE_ROWS], y.reshape(-1).numpy()[keep][:SAMPLE_ROWS]
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        dump_svmlight_file(xs, ys, where, query_id=np.zeros(len(ys), dtype=np.int64))
        out.append(time.perf_counter() - t0)
    os.remove(where)
    return statistics.median(out), len(ys)


def measure(name, args, dev, workdir):
    x, y = make_chunk(name, args.scale, 7)
    n = x.shape[0]
    rows = n * L
    kept = int((y != -1).sum())
    xd, yd = x.reshape(rows, F).to(dev), y.reshape(rows).to(dev)
    qd = torch.arange(n, device=dev).repeat_interleave(L)
    lib, st = LB.lib(), LB.launch_stream(dev)
    line_bytes = torch.empty(rows, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    S.libsvm_line_bytes(lib, st, xd, yd, qd, -1.0, 0, line_bytes, bad)
    end = torch.cumsum(line_bytes, 0)
    total = int(end[-1])
    start = end - line_bytes
    text, spare = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(total, dtype=torch.uint8, device=dev)
    slates_x, slates_y = list(x), list(y)                     # the reference's argument form: CPU tensors per slate
    target = os.path.join(workdir, name + ".svm")

    def end_to_end():
        t0 = time.perf_counter()
        S.write_to_libsvm_without_masked(target, slates_x, slates_y)
        return (time.perf_counter() - t0) * 1e3

    arms = {"pass A (line_bytes)": lambda: timed(lambda: S.libsvm_line_bytes(lib, st, xd, yd, qd, -1.0, 0, line_bytes, bad)),
            "pass B (format)": lambda: timed(lambda: S.libsvm_format(lib, st, xd, yd, qd, -1.0, 0, start, text)),
            "device-to-device copy of the text": lambda: timed(lambda: spare.copy_(text)),
            "write_to_libsvm_without_masked, end to end": end_to_end}
    times = {k: [] for k in arms}
    for rnd in range(3 + args.runs):
        for k, fn in arms.items():
            ms = fn()
            if rnd >= 3:
                times[k].append(ms)
        print("%s: round %d of %d" % (name, rnd + 1, 3 + args.runs), flush=True)
    assert S.last_run["engine"] == "device" and S.last_run["bytes"] == total and os.path.getsize(target) == total
    os.remove(target)
    sk, sk_rows = sklearn_seconds(x, y, os.path.join(workdir, name + ".sklearn.svm"))
    return dict(name=name, slates=n, rows=rows, kept=kept, values=kept * F, total=total, times=times, sklearn=sk, sklearn_rows=sk_rows)


def table(m):
    lines = ["## %s: %d slates x %d slots, %d rows kept, %.1f M values, %.1f MB of text (%.1f bytes per value)"
             % (m["name"], m["slates"], L, m["kept"], m["values"] / 1e6, m["total"] / 1e6, m["total"] / m["values"]),
             "",
             "| arm | time, ms | text GB/s | M values/s |",
             "|---|---|---|---|"]
    for k, v in m["times"].items():
        med = statistics.median(v)
        lines.append("| %s | %.3f (%.1f %%) | %.2f | %.0f |" % (k, med, 100 * (max(v) - min(v)) / med, m["total"] / (med * 1e-3) / 1e9,
                                                              m["values"] / (med * 1e-3) / 1e6))
    if m["sklearn"] is None:
        lines.append("| scikit-learn dump_svmlight_file | not measured: scikit-learn does not import on this host (the only figure there is: "
                     "1.9 M values/s, 43 MB/s, in a CPU container) | | |")
    else:
        full = m["sklearn"] * m["kept"] / m["sklearn_rows"]
        lines.append("| scikit-learn dump_svmlight_file, %d-row sample (measured, 3 runs) | %.0f | %.3f | %.1f |"
                     % (m["sklearn_rows"], m["sklearn"] * 1e3, m["total"] * m["sklearn_rows"] / m["kept"] / m["sklearn"] / 1e9,
                        m["sklearn_rows"] * F / m["sklearn"] / 1e6))
        lines.append("| scikit-learn, all %d rows (SCALED from the sample by the row count, not measured) | %.0f | | |" % (m["kept"], full * 1e3))
        e2e = statistics.median(m["times"]["write_to_libsvm_without_masked, end to end"]) * 1e-3
        lines += ["", "End to end against scikit-learn's scaled figure on the same host and arrays: %.1f x %s."
                  % (max(full / e2e, e2e / full), "faster" if e2e < full else "SLOWER")]
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svm_write.md"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--dir", default=None, help="where the files are written (default: the system's temporary directory)")
    ap.add_argument("--scale", type=float, default=1.0, help="slate counts x this (rehearsals)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_svm_write.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory(dir=args.dir) as workdir:
        fs = file_system_of(workdir)
        results = [measure(name, args, dev, workdir) for name in ("web30k-vali", "dense")]
    lines = ["# libsvm text written on the device: the two passes, a copy of the same bytes, the writer end to end",
             "",
             "Written by `tools/time_svm_write.py` (its docstring says what the arms are and how the windows are taken).  %s, ROCm torch %s."
             % (torch.cuda.get_device_name(0), torch.__version__),
             "fp32 standard normals, F = %d.  Kernel arms: device events; end to end: a host clock around the call, files on %s." % (F, fs),
             "3 warm-up rounds, medians of %d rounds, the spread of the rounds in brackets.  GB/s = bytes of text over the time." % args.runs,
             ""]
    for m in results:
        lines += table(m)
    lines += ["Both passes run the exact formatter on every non-zero value (multi-word integer arithmetic, no floating point); the copy of the",
              "same bytes is what a pure data mover reaches.  What bounds the passes has not been checked with counters, and whether a first",
              "pass that stored token lengths for the second would pay has not been measured.", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
