"""Table of the attention kernels' resource usage from hipcc's remarks, for comparing two trees (profiles/attention_m16_resources.md).
Compiles csrc/attention_bf16.hip and csrc/attention_fp8.hip of each tree for gfx950 (no GPU needed) with -Rpass-analysis=kernel-resource-usage.
usage: python tools/kernel_resources.py PARENT_TREE [THIS_TREE]      (a tree = a directory that holds thinkdiff-mlre_amd/ and include/)"""
import os
import re
import subprocess
import sys
import tempfile

FILES = ("attention_bf16.hip", "attention_fp8.hip")
KEYS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("VGPRs Spill", "vgpr spill"), ("SGPRs Spill", "sgpr spill"),
        ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "lds"))


def remarks(tree):
    out = {}
    for f in FILES:
        src = os.path.join(tree, "thinkdiff-mlre_amd", "csrc", f)
        with tempfile.TemporaryDirectory() as tmp:
            err = subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                                  os.path.join(tmp, "x.o")], check=True, capture_output=True, text=True).stderr
        name = None
        for line in err.splitlines():
            m = re.search(r"remark: (?:.*?: )?Function Name: (\S+)", line)
            if m:
                name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
                name = re.sub(r"^void ", "", name).split("(")[0]
                out[name] = {}
                continue
            for key, short in KEYS:
                m = re.search(r"remark: (?:.*?: )?\s*" + re.escape(key) + r": (\d+)", line)
                if m and name:
                    out[name][short] = int(m.group(1))
    return out


def main():
    parent = remarks(sys.argv[1])
    here = remarks(sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    cols = [s for _, s in KEYS]
    print("| kernel | " + " | ".join(cols) + " | against the parent |")
    print("|---|" + "---|" * (len(cols) + 1))
    for name in sorted(here):
        h, p = here[name], parent.get(name)
        if p is None and name.endswith(", false>"):      # a template parameter added at the end, default false
            p = parent.get(name[:-len(", false>")] + ">")
        note = "new" if p is None else ("identical" if p == h else "CHANGED: parent " + ", ".join(f"{c} {p.get(c)}" for c in cols if p.get(c) != h.get(c)))
        print(f"| `{name}` | " + " | ".join(str(h.get(c, "")) for c in cols) + f" | {note} |")
    for name in sorted(set(parent) - set(here)):
        print(f"| `{name}` | " + " | ".join("" for _ in cols) + " | REMOVED |")


if __name__ == "__main__":
    main()
