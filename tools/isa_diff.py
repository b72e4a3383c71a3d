"""Whether two source trees compile to the same gfx950 device code, kernel by
kernel: the check a refactor of the kernel units has to pass. CPU only.

  python3 tools/isa_diff.py OLD_TREE NEW_TREE [--only UNIT.hip ...] [--rename REGEX=REPLACEMENT ...]

Every .hip unit under each tree's multiraft_amd/csrc is compiled to device
assembly (the Makefile's HIPFLAGS of that tree plus --offload-device-only -S,
at most 16 compiler processes, output in a temporary directory). Each kernel is
cut from its symbol label to its .Lfunc_end, which takes in its kernel
descriptor, and joined with its resource lines of the code object's metadata
(register and spill counts, LDS, scratch and kernel-argument sizes). Comments
go; the function number in local labels and the per-build unit id are
normalised. A kernel is named by its demangled name without the parameter
list, so a kernel may move to another unit, or a parameter type to another
namespace, and still be matched. Prints IDENTICAL / DIFFERS / ONLY-IN-ONE per
kernel; exits 0 only when both trees hold the same kernels, all identical.
--rename REGEX=REPLACEMENT (repeatable, re.sub on the old tree's kernel names
before matching) pairs a kernel the new tree renamed with its old self.

The old tree is usually the parent commit:
  git archive HEAD | tar -x -C /tmp/parent
The tool compares text; it names no instruction and searches for none."""
from __future__ import annotations

import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join("multiraft_amd", "csrc")
JOBS = 16
RESOURCES = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".kernarg_segment_size", ".vgpr_spill_count", ".sgpr_spill_count")


def hipflags(csrc: str) -> list[str]:
    """HIPFLAGS of the tree's Makefile, ARCH at its default."""
    text = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*:?=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\??=\s*(\S+)", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def compile_asm(src: str, out: str) -> str:
    cmd = [HIPCC, *hipflags(os.path.dirname(src)), "--offload-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(f"{src} did not compile:\n{r.stderr[-3000:]}")
    return open(out).read()


def demangle(symbols: list[str]) -> list[str]:
    if not symbols:
        return []
    r = subprocess.run(["c++filt"], input="\n".join(symbols) + "\n", capture_output=True, text=True, check=True)
    return r.stdout.splitlines()


def kernel_name(demangled: str) -> str:
    """`void ns::k<1, 2>(ns::T, int*)` -> `ns::k<1, 2>`: the name without return type and parameters."""
    s = demangled.strip()
    if s.endswith(")"):
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += s[i] == ")"
            depth -= s[i] == "("
            if depth == 0:
                s = s[:i]
                break
    return s[5:] if s.startswith("void ") else s


def normalise(text: str, symbol: str = "") -> list[str]:
    """The lines of a piece of assembly that decide its code: comments and
    blank lines dropped, the function number of local labels, the unit id and
    the kernel's own symbol replaced by fixed words."""
    out = []
    for line in text.splitlines():
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        if symbol:
            line = line.replace(symbol, "<kernel>")
        line = re.sub(r"\.LBB\d+_", ".LBB<f>_", line)
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1<f>", line)
        line = re.sub(r"__hip_cuid_\w+", "__hip_cuid_<id>", line)
        out.append(line)
    return out


def kernels_of(asm: str) -> dict[str, list[str]]:
    """name -> normalised body and resource lines, for every kernel of one unit's assembly."""
    symbols = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    meta = {}
    for entry in re.split(r"^  - (?=\.agpr_count|\.args)", asm.split("amdhsa.kernels:", 1)[-1], flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M)
        if name:
            meta[name.group(1)] = [m.group(0).strip() for key in RESOURCES
                                   for m in [re.search(rf"^\s+{re.escape(key)}:\s+\S+", entry, re.M)] if m]
    lines = asm.splitlines()
    out = {}
    for sym, name in zip(symbols, map(kernel_name, demangle(symbols))):
        start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        out[name] = normalise("\n".join(lines[start:end + 1]), sym) + meta.get(sym, [])
    return out


def tree_kernels(tree: str, tmp: str, tag: str, only: list[str]) -> dict[str, tuple[str, list[str]]]:
    """name -> (unit, lines) for every kernel of the tree."""
    csrc = os.path.join(tree, CSRC)
    srcs = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    if only:
        srcs = [s for s in srcs if os.path.basename(s) in only]
    with ThreadPoolExecutor(JOBS) as ex:
        asms = list(ex.map(lambda s: compile_asm(s, os.path.join(tmp, f"{tag}_{os.path.basename(s)}.s")), srcs))
    out = {}
    for src, asm in zip(srcs, asms):
        for name, body in kernels_of(asm).items():
            if name in out:
                raise RuntimeError(f"{name} is defined in {out[name][0]} and {os.path.basename(src)}")
            out[name] = (os.path.basename(src), body)
    return out


def compare(old: dict, new: dict) -> list[tuple[str, str]]:
    rows = []
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            rows.append(("ONLY-IN-ONE", f"{name}  ({'old' if name in old else 'new'}: {(old.get(name) or new[name])[0]})"))
        else:
            (uo, bo), (un, bn) = old[name], new[name]
            where = uo if uo == un else f"{uo} -> {un}"
            rows.append(("IDENTICAL" if bo == bn else "DIFFERS", f"{name}  ({where})"))
    return rows


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--only", nargs="*", default=[], help="unit file names to compare (default: every .hip unit)")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPLACEMENT",
                    help="applied to the old tree's kernel names before matching (repeatable)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old = tree_kernels(a.old_tree, tmp, "old", a.only)
        new = tree_kernels(a.new_tree, tmp, "new", a.only)
    for pattern, replacement in (r.split("=", 1) for r in a.rename):
        renamed = {re.sub(pattern, replacement, name): kernel for name, kernel in old.items()}
        if len(renamed) != len(old):
            raise RuntimeError(f"--rename {pattern}={replacement} maps two kernels of the old tree to one name")
        old = renamed
    rows = compare(old, new)
    for verdict, what in rows:
        print(f"{verdict:12s}{what}")
    n = {v: sum(1 for r in rows if r[0] == v) for v in ("IDENTICAL", "DIFFERS", "ONLY-IN-ONE")}
    print(f"{len(rows)} kernels: {n['IDENTICAL']} identical, {n['DIFFERS']} differ, {n['ONLY-IN-ONE']} only in one tree")
    return 0 if rows and n["IDENTICAL"] == len(rows) else 1


if __name__ == "__main__":
    sys.exit(main())
