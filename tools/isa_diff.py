#!/usr/bin/env python3
"""Compare the gfx950 code of two source trees, function by function.

    python tools/isa_diff.py OLD_TREE NEW_TREE [--out DIR] [--reuse] [--jobs N]

Every lac_amd/csrc/*.hip of both trees is compiled to assembly with the flags and
include paths of that tree's lac_amd/build.py plus `--cuda-device-only -S`, into
DIR/old and DIR/new (a temporary directory by default; never inside the trees).
Each file is split by function symbol (`.type NAME,@function`), and for every
mangled name three texts are compared: the instructions, the kernel's .amdhsa_*
descriptor block, and its entry in the code object's metadata (VGPRs, SGPRs,
scratch, LDS, arguments).  Lines naming the `__hip_cuid_` symbol -- a hash of the
source text -- are dropped, data symbols are ignored, and the function ordinal in
local labels (.LBB<n>_<m>, .Lfunc_end<n>) is blanked, so that moving a kernel in
its file does not count.  The tool compares text: it looks for no instruction.

Prints per unit how many functions are identical, differ (with both line counts)
or exist in one tree only; exits 0 only if every function of every unit is
identical and both trees define the same names.  A refactor that must not change
speed is checked against a `git worktree` of its parent commit:

    git worktree add /tmp/parent HEAD && python tools/isa_diff.py /tmp/parent .

--reuse keeps an assembly file that is newer than every source of its tree, which
saves recompiling the old side on each run.
"""
from __future__ import annotations

import argparse
import glob
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

MAX_JOBS = 16
_TYPE_FN = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
_TYPE_ANY = re.compile(r"^\s*\.type\s+([^\s,]+),@")
_ORDINAL = re.compile(r"(\.L[A-Za-z]+)\d+(_\d+)\b|(\.Lfunc_(?:begin|end))\d+\b")
_META_NAME = re.compile(r"^\s+\.name:\s+(\S+)\s*$")


def _norm(line: str) -> str:
    return _ORDINAL.sub(lambda m: m.group(1) + m.group(2) if m.group(1) else m.group(3), line.rstrip())


def split_functions(text: str) -> dict:
    """{mangled name: {"code": [...], "desc": [...], "meta": [...]}} of one assembly file."""
    lines = [ln for ln in text.splitlines() if "__hip_cuid_" not in ln]
    try:
        meta_at = next(i for i, ln in enumerate(lines) if ln.strip() == ".amdgpu_metadata")
    except StopIteration:
        meta_at = len(lines)
    out, cur, in_desc = {}, None, False
    for ln in lines[:meta_at]:
        m = _TYPE_ANY.match(ln)
        if m:  # a new symbol: a function opens a record, a data symbol closes the last one
            fn = _TYPE_FN.match(ln)
            cur = out.setdefault(fn.group(1), {"code": [], "desc": [], "meta": []}) if fn else None
            in_desc = False
            continue
        if cur is None or not ln.strip():
            continue
        s = ln.strip()
        if s.endswith("-- End function"):  # what follows is the next symbol's preamble
            cur = None
            continue
        if s.startswith(".amdhsa_kernel "):
            in_desc = True
        elif s == ".end_amdhsa_kernel":
            in_desc = False
        elif in_desc:
            cur["desc"].append(s)
        else:
            cur["code"].append(_norm(ln))
    # metadata: one YAML list item ("  - .key: ...") per kernel under amdhsa.kernels
    item = []
    def close():
        for ln in item:
            m = _META_NAME.match(ln)
            if m and m.group(1) in out:
                out[m.group(1)]["meta"] = [x.rstrip() for x in item]
    for ln in lines[meta_at:]:
        if ln.startswith("  - ") or not ln.startswith(" "):
            close()
            item = []
        if ln.startswith(" "):
            item.append(ln)
    close()
    return out


def compare(old: dict, new: dict) -> dict:
    """Names sorted into identical / differing (with what differs and line counts) / one-sided."""
    res = {"identical": [], "differing": [], "only_old": sorted(set(old) - set(new)),
           "only_new": sorted(set(new) - set(old))}
    for name in sorted(set(old) & set(new)):
        parts = [p for p in ("code", "desc", "meta") if old[name][p] != new[name][p]]
        if parts:
            res["differing"].append((name, parts, len(old[name]["code"]), len(new[name]["code"])))
        else:
            res["identical"].append(name)
    return res


def all_identical(res: dict) -> bool:
    return not (res["differing"] or res["only_old"] or res["only_new"])


def _build_module(tree: str):
    spec = importlib.util.spec_from_file_location("_isa_diff_build_" + str(abs(hash(tree))),
                                                  os.path.join(tree, "lac_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def asm_jobs(tree: str, outdir: str, reuse: bool) -> tuple:
    """({unit: assembly path}, [compile commands still to run]) for one tree."""
    tree = os.path.abspath(tree)
    b = _build_module(tree)
    os.makedirs(outdir, exist_ok=True)
    deps = [*glob.glob(os.path.join(tree, "lac_amd", "csrc", "*")), *glob.glob(os.path.join(tree, "include", "*.h"))]
    paths, cmds = {}, []
    for src in sorted(glob.glob(os.path.join(tree, "lac_amd", "csrc", "*.hip"))):
        unit = os.path.basename(src)[:-4]
        s = paths[unit] = os.path.join(outdir, unit + ".s")
        fresh = reuse and os.path.exists(s) and all(os.path.getmtime(d) < os.path.getmtime(s) for d in deps)
        if not fresh:
            cmds.append(["hipcc", *b.FLAGS, *b._incs(), "--cuda-device-only", "-S", src, "-o", s])
    return paths, cmds


def run_compiles(cmds: list, jobs: int) -> None:
    if not cmds:
        return
    with ThreadPoolExecutor(max(1, min(jobs, MAX_JOBS, len(cmds)))) as ex:
        procs = list(ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), cmds))
    for c, p in zip(cmds, procs):
        if p.returncode:
            sys.stderr.write(p.stderr)
            raise SystemExit("compile failed: " + " ".join(c))


def _short(name: str, n: int = 110) -> str:
    return name if len(name) <= n else name[:n] + "..."


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--out", help="directory for the assembly (default: a temporary one)")
    ap.add_argument("--reuse", action="store_true", help="keep assembly newer than its tree's sources")
    ap.add_argument("--jobs", type=int, default=MAX_JOBS, help=f"parallel compiles, at most {MAX_JOBS}")
    a = ap.parse_args(argv)
    tmp = None
    if not a.out:
        tmp = tempfile.TemporaryDirectory(prefix="isa_diff_")
        a.out = tmp.name
    for tree in (a.old_tree, a.new_tree):
        if os.path.commonpath([os.path.abspath(a.out), os.path.abspath(tree)]) == os.path.abspath(tree):
            raise SystemExit("--out must lie outside both trees")
    old_s, c1 = asm_jobs(a.old_tree, os.path.join(a.out, "old"), a.reuse)
    new_s, c2 = asm_jobs(a.new_tree, os.path.join(a.out, "new"), a.reuse)
    run_compiles(c1 + c2, a.jobs)
    ok = True
    print("| unit | functions | identical | differing | only old | only new |")
    print("|---|---|---|---|---|---|")
    details = []
    for unit in sorted(set(old_s) | set(new_s)):
        if unit not in old_s or unit not in new_s:
            ok = False
            print(f"| {unit} | present in {'old' if unit in old_s else 'new'} tree only | | | | |")
            continue
        with open(old_s[unit]) as f:
            o = split_functions(f.read())
        with open(new_s[unit]) as f:
            n = split_functions(f.read())
        res = compare(o, n)
        ok = ok and all_identical(res)
        print(f"| {unit} | {len(set(o) | set(n))} | {len(res['identical'])} | {len(res['differing'])} "
              f"| {len(res['only_old'])} | {len(res['only_new'])} |")
        details += [f"DIFF  {unit}: {'+'.join(parts)} {lo} -> {ln} lines  {_short(name)}"
                    for name, parts, lo, ln in res["differing"]]
        details += [f"ONLY-OLD  {unit}: {_short(x)}" for x in res["only_old"]]
        details += [f"ONLY-NEW  {unit}: {_short(x)}" for x in res["only_new"]]
    print()
    for d in details:
        print(d)
    print("all functions identical, name sets equal" if ok else "NOT identical")
    if tmp:
        tmp.cleanup()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
