"""Plain text comparison of two builds of the library's device assembly, kernel by kernel.

    for f in allrank_amd/csrc/*.hip; do
        hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S $f -o DIR/$(basename $f).s
    done                                              # once in the parent's tree (DIR = A), once in this one (DIR = B)
    python tools/asm_compare.py A B

Per kernel it compares the function body, the `.amdhsa_kernel` descriptor and the metadata entry, after normalising the
`__hip_cuid_*` id and the function index inside local labels (`.LBBn_m`, `BBn_m`, `.Lfunc_endn`, `.LJTIn_m`), which moves when
functions are reordered in a file.  Exit status 0 when every kernel of every file is identical.
"""
import os
import re
import sys


def kernels(path):
    t = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:\n", t, re.S | re.M):
        body = re.sub(r"\.?LBB\d+_(\d+)", r"LBBn_\1", m.group(2))
        body = re.sub(r"\bBB\d+_(\d+)", r"BBn_\1", body)
        body = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1n", body)
        out.setdefault(m.group(1), {})["body"] = re.sub(r"\.LJTI\d+_(\d+)", r".LJTIn_\1", body)
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\w+)\n(.*?)^\s*\.end_amdhsa_kernel", t, re.S | re.M):
        out.setdefault(m.group(1), {})["descriptor"] = m.group(2)
    meta = t[t.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in t else ""
    for e in re.split(r"^  - \.agpr_count:", meta, flags=re.M)[1:]:
        e = e.split("amdhsa.target:")[0]
        out.setdefault(re.search(r"\.name:\s+(\w+)", e).group(1), {})["metadata"] = e
    out = {k: v for k, v in out.items() if "descriptor" in v}           # kernels only, not the device functions
    for k, v in out.items():
        assert set(v) == {"body", "descriptor", "metadata"}, (path, k, sorted(v))
    return out


def main(a_dir, b_dir):
    total = differing = 0
    for f in sorted(set(os.listdir(a_dir)) | set(os.listdir(b_dir))):
        ka, kb = kernels(os.path.join(a_dir, f)), kernels(os.path.join(b_dir, f))
        diff = [k for k in sorted(set(ka) | set(kb)) if ka.get(k) != kb.get(k)]
        total += len(kb)
        differing += len(diff)
        print("%-30s kernels %3d / %3d   differing %d" % (f, len(ka), len(kb), len(diff)))
        for k in diff:
            print("    %s: %s" % (k, ", ".join(p for p in ("body", "descriptor", "metadata") if ka.get(k, {}).get(p) != kb.get(k, {}).get(p))))
    print("total %d kernels, %d differing" % (total, differing))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
