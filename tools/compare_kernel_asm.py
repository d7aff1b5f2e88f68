"""Per-kernel comparison of two device assembly files of one source at two commits, CPU only.

  hipcc --offload-arch=gfx950 <CXXFLAGS of csrc/Makefile> -S --cuda-device-only -o before.s csrc/ist_png_deflate.hip   (at the parent)
  hipcc --offload-arch=gfx950 <CXXFLAGS of csrc/Makefile> -S --cuda-device-only -o after.s  csrc/ist_png_deflate.hip   (at the branch)
  python tools/compare_kernel_asm.py before.s after.s

A kernel's instruction stream is the lines between its label and its .Lfunc_end, with comments and directives stripped and the
function number taken out of the block labels.  One line per kernel: identical or CHANGED, the instruction counts, and for a changed
kernel the register, LDS and private-segment figures of both files' metadata.  Exit status 1 when a kernel named by --pinned
(a substring, may be given more than once) is not identical.
"""
import argparse
import re
import sys

KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def short(name):
    m = re.search(r"\d+(ist_\w+?_kernel)E", name)
    return m.group(1) if name.startswith("_Z") and m else name


def kernels(path):
    text = open(path).read()
    streams, name, cur = {}, None, None
    for ln in text.split("\n"):
        m = re.match(r"^(\w+):\s*(;.*)?$", ln)
        if m and name is None and re.search(r"ist_\w+_kernel", m.group(1)) and not m.group(1).startswith("__"):
            name, cur = short(m.group(1)), []
            continue
        if name is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", ln):
            streams[name], name = cur, None
            continue
        s = ln.split(";")[0].strip()
        if not s or (s.startswith(".") and not re.match(r"^\.L\w+:$", s)):
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        nm = re.search(r"\.name:\s+(\w+)", blk)
        if nm:
            meta[short(nm.group(1))] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", blk).group(1)) for k in KEYS if re.search(re.escape(k) + r":\s+\d+", blk)}
    return streams, meta


def count(stream):
    return sum(1 for s in stream if not s.endswith(":"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--pinned", action="append", default=[])
    a = ap.parse_args()
    (sa, ma), (sb, mb) = kernels(a.before), kernels(a.after)
    bad = 0
    for k in sorted(set(sa) | set(sb)):
        if k not in sa or k not in sb:
            print("%-44s only in %s" % (k, a.before if k in sa else a.after))
            same = False
        else:
            same = sa[k] == sb[k]
            line = "%-44s %s  %d -> %d instructions" % (k, "identical" if same else "CHANGED  ", count(sa[k]), count(sb[k]))
            if not same:
                line += "\n    before %s\n    after  %s" % (ma.get(k), mb.get(k))
            print(line)
        if not same and any(p in k for p in a.pinned):
            bad = 1
    return bad


if __name__ == "__main__":
    sys.exit(main())
