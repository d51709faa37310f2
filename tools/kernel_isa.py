#!/usr/bin/env python3
"""Compare the gfx950 code of every kernel in a .hip file with a git revision.

    tools/kernel_isa.py FILE.hip [--base REV] [--rename OLD=NEW]...

Compiles the working-tree FILE and the copy of it in REV (default HEAD; the
whole ops/csrc directory is extracted, so headers come along) to device
assembly with the flags of ops/build.py and prints, per kernel, same / DIFF /
added / removed plus both versions' register, spill, scratch, occupancy and
LDS figures. Exits non-zero if a kernel present on both sides differs. Run it
after every kernel edit: a refactor must leave every kernel `same`.

Kernels are paired by symbol. --rename pairs a kernel of REV with the
working-tree kernel whose demangled name is REV's with the regular expression
OLD replaced by NEW, e.g. for a renamed template with one more argument
    --rename 'old_kernel<(.*)>=new_kernel<\1, false>'
"""

from __future__ import annotations

import argparse
import io
import os
import re
import shutil
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_REL = "zero_transformer_amd/ops/csrc"

# resource remark label -> column name
FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("SGPRs Spill", "sspill"),
          ("VGPRs Spill", "vspill"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds")]


def kernels(asm: str) -> dict:
    """symbol -> normalised instruction text of every function in `asm`."""
    out = {}
    for sym in re.findall(r"^\s*\.type\s+([^\s,]+),@function", asm, re.M):
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), asm, re.M | re.S)
        if not m:
            continue
        lines = []
        for line in m.group(1).splitlines():
            line = line.split(";", 1)[0].strip()
            if not line or (line.startswith(".") and not line.endswith(":")):
                continue  # comment, blank or assembler directive
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        out[sym] = "\n".join(lines)
    return out


def compare(base: dict, new: dict) -> dict:
    """symbol -> 'same' | 'DIFF' | 'added' | 'removed'."""
    res = {}
    for sym in sorted(set(base) | set(new)):
        if sym not in base:
            res[sym] = "added"
        elif sym not in new:
            res[sym] = "removed"
        else:
            res[sym] = "same" if base[sym] == new[sym] else "DIFF"
    return res


def renamed(base, new, names: dict, renames: list) -> dict:
    """base symbol -> the symbol in `new` that carries its name after the
    (old regex, replacement) pairs in `renames`, for every base symbol whose
    name they change and that has such a counterpart. names: symbol ->
    demangled name."""
    by_name = {names[s]: s for s in new}
    out = {}
    for sym in base:
        name = names[sym]
        for old, repl in renames:
            name = re.sub(old, repl, name)
        if name != names[sym] and name in by_name:
            if by_name[name] in base:
                sys.exit(f"--rename maps {names[sym]} onto {name}, which the base has too")
            out[sym] = by_name[name]
    return out


def rename_arg(s: str) -> tuple:
    old, new = s.split("=", 1)  # ValueError without "=": argparse reports it
    return old, new


def resources(remarks: str) -> dict:
    """symbol -> {column: value} from -Rpass-analysis=kernel-resource-usage."""
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur.update({col: m.group(2) for label, col in FIELDS if label == m.group(1)})
    return out


def compile_asm(src: str) -> tuple:
    from zero_transformer_amd.ops.build import hipcc_compile_cmd

    cmd = hipcc_compile_cmd() + ["--cuda-device-only", "-S",
                                 "-Rpass-analysis=kernel-resource-usage", src, "-o", "-"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode:
        sys.exit(f"hipcc failed on {src}:\n{p.stderr[-4000:]}")
    return kernels(p.stdout), resources(p.stderr)


def demangle(syms: list) -> dict:
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt or not syms:
        return {s: s for s in syms}
    names = subprocess.run([filt, "-p"] + syms, capture_output=True, text=True).stdout.split("\n")
    return dict(zip(syms, names))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("file")
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    type=rename_arg)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    rel = os.path.relpath(os.path.abspath(a.file), ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.base, CSRC_REL],
                             capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        old = os.path.join(tmp, rel)
        with ThreadPoolExecutor(max_workers=2) as ex:  # at most two hipcc at a time
            fb = ex.submit(compile_asm, old) if os.path.exists(old) else None
            new, new_res = ex.submit(compile_asm, os.path.join(ROOT, rel)).result()
            base, base_res = fb.result() if fb else ({}, {})
    names = demangle(sorted(set(base) | set(new)))
    to = renamed(base, new, names, a.rename)
    was = {n: f" (was {names[b]})" for b, n in to.items()}
    base, base_res = ({to.get(s, s): v for s, v in d.items()} for d in (base, base_res))
    status = compare(base, new)
    print(f"{rel}: working tree vs {a.base}   (" + " ".join(c for _, c in FIELDS) + "; base -> new)")
    for sym, st in status.items():
        cols = ["/".join(r.get(sym, {}).get(c, "-") for _, c in FIELDS)
                + f" {k[sym].count(chr(10)) + 1 if sym in k else '-'} lines"
                for r, k in ((base_res, base), (new_res, new))]
        print(f"{st:8s}{names[sym]}{was.get(sym, '')}:  {cols[0]} -> {cols[1]}")
    return int("DIFF" in status.values())


if __name__ == "__main__":
    sys.exit(main())
