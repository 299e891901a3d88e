"""Record what the host-side GEMM planning exports of libltrx return over a grid of shapes (no GPU needed).

    python tests/golden/make_gemm_plan_fixture.py [--out FILE]

Writes tests/golden/gemm_plan_parent.json: for every shape of the grid the values of ltrx_gemm_tn_splits,
ltrx_gemm_tn_workspace_bytes, ltrx_gemm_tn_group_workspace_bytes, ltrx_gemm_nt_relu_bits_bytes, ltrx_debug_tn_group_map and
ltrx_debug_tn_group_side_plan of the library built from the checked-out tree.  It was run ONCE, at the commit named in the file
("commit"), before the host part of allrank_amd/csrc/ltrx_gemm.hip was rewritten around launch plans; tests/test_gemm_plan_cpu.py
holds every later library to these values exactly.  Re-running it at a later commit only re-records that commit against itself.

The grid: the bench layer (d 512, d_ff 2048) at 61440 and 15360 rows, the padded-input shapes (136 and 46 features in rows of 256
floats), row counts on both sides of 2048 and of the % 32 / % 128 boundaries next to it, tile counts on both sides of every threshold
of the NT dispatch (136, 168, 176, 256, 360, 380 tiles of 256, 128 and 64 rows), and the compositions a layer's weight gradients
are grouped in (all four, and two by two when both sublayer dropouts are on).  Tables of bytes are recorded as their CRC-32.
"""
import ctypes
import json
import os
import subprocess
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

D, DFF = 512, 2048
W2, W1, WO, WQ = (D, DFF), (DFF, D), (D, D), (3 * D, D)
ROWS = [1, 31, 32, 33, 127, 128, 129, 511, 512, 2016, 2047, 2048, 2049, 2079, 2080, 2081, 2175, 2176, 2177, 4064, 4096, 4128,
        15359, 15360, 15361, 15392, 61312, 61408, 61439, 61440, 61441]
TN_SHAPES = [WQ, WO, W1, W2, (512, 136), (512, 46), (512, 256), (1, 512), (96, 136), (256, 256), (768, 256), (130, 70), (1024, 1024),
             (4096, 4096), (4096, 4352), (256, 4), (512, 48)]
GROUPS = [[W2, W1, WO, WQ], [W2, W1], [WO, WQ], [W2], [W1], [WO], [WQ], [(256, 256)] * 4, [(256, 256)], [(96, 136)], [(512, 136)],
          [(512, 256), (512, 512)], [(1024, 1024)] * 4, [(4096, 4096)], [(4096, 4096), (256, 256)], [(2048, 2048)] * 3]
# (rows, D, has_dres, side_wgs) of the LayerNorm side job asked about with every group; rows 0 = the group's own row count
SIDE_JOBS = [(0, 512, 1, 0), (0, 512, 0, 0), (0, 512, 1, 8), (0, 384, 1, 0), (61440, 1024, 1, 0)]
NT_THRESHOLDS = [136, 168, 176, 256, 360, 380, 512]
NT_COLS = [256 * nn for nn in (1, 2, 8, 130, 150, 256, 300)] + [300]
NT_K = [32, 48, 2048]


def nt_rows(nn):
    """row counts that put ceil(M / bm) * nn on both sides of every threshold, for the three tile heights"""
    out = set()
    for b in NT_THRESHOLDS:
        for bm in (256, 128, 64):
            k = -(-b // nn)
            out.update(m for m in (bm * (k - 1), bm * (k - 1) + 1, bm * k, bm * k + 1) if m > 0)
    return sorted(out)


def crc(buf, n):
    return zlib.crc32(bytes(bytearray(buf)[:n]))


def record(lib):
    tn = [[M, NP, KP, lib.ltrx_gemm_tn_splits(M, NP, KP), lib.ltrx_gemm_tn_workspace_bytes(M, NP, KP)]
          for (NP, KP) in TN_SHAPES for M in ROWS]
    bits = [[M, N, K, lib.ltrx_gemm_nt_relu_bits_bytes(M, N, K)]
            for N in NT_COLS for K in NT_K for M in nt_rows(max(N // 256, 1))]
    groups = []
    for probs in GROUPS:
        n = len(probs)
        NP = (ctypes.c_int * n)(*[a for a, _ in probs])
        KP = (ctypes.c_int * n)(*[b for _, b in probs])
        for M in ROWS:
            t_out, s_out = (ctypes.c_ubyte * 256)(), (ctypes.c_ubyte * 256)()
            wgs = lib.ltrx_debug_tn_group_map(n, M, NP, KP, t_out, s_out)
            side = []
            for (rows, d, dres, sw) in SIDE_JOBS:
                gemm, vbl, owner = ctypes.c_int(-1), ctypes.c_int(-1), (ctypes.c_int * 320)()
                taken = lib.ltrx_debug_tn_group_side_plan(n, M, NP, KP, rows or M, d, dres, sw, ctypes.byref(gemm), ctypes.byref(vbl), owner)
                side.append([rows or M, d, dres, sw, taken, gemm.value, vbl.value, crc(owner, 4 * 320)])
            groups.append(dict(M=M, probs=[list(p) for p in probs], ws_bytes=lib.ltrx_gemm_tn_group_workspace_bytes(n, M, NP, KP),
                               wgs=wgs, tile_crc=crc(t_out, wgs), split_crc=crc(s_out, wgs), side=side))
    return dict(tn=tn, relu_bits=bits, groups=groups)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "gemm_plan_parent.json"))
    args = ap.parse_args()
    from allrank_amd import _lib, build
    build.build(verbose=False)
    rec = record(_lib.lib())
    commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"]).decode().strip()
    dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "allrank_amd/csrc", "include"]).decode().strip()
    with open(args.out, "w") as fh:                       # one row per line: a change of one value is a one-line diff
        fh.write('{"commit": %s,\n "library_sources_modified": %s' % (json.dumps(commit), json.dumps(bool(dirty))))
        for key in ("tn", "relu_bits", "groups"):
            fh.write(',\n "%s": [\n  %s\n ]' % (key, ",\n  ".join(json.dumps(r) for r in rec[key])))
        fh.write("\n}\n")
    print("wrote %s: %s" % (args.out, ", ".join("%d %s" % (len(rec[k]), k) for k in ("tn", "relu_bits", "groups"))))


if __name__ == "__main__":
    main()
