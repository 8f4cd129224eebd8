#!/usr/bin/env python3
"""Is the gfx950 device code of this tree the same as that of another commit?

For a change that only renames and re-files device code.  Each HIP translation unit of the library
(the objects that the Makefile links into it) is compiled to device assembly (the Makefile's HIPFLAGS plus -I../../include --offload-device-only -S)
from a `git archive` of the other commit and from the working tree, and the two texts are compared
line for line after the one symbol that hashes the source text, __hip_cuid_<hash>, is replaced by a
fixed word.  Needs hipcc and no GPU; about 35 s per unit and side.

    python3 profiles/scripts/compare_device_asm.py [COMMIT] [--keep DIR] > profiles/region_names.txt

COMMIT defaults to HEAD^.  With --keep the assembly stays in DIR, and the other commit's side is
reused from there on the next call.  Prints the verdict per unit and, for a unit that differs, the
functions that hold the differing lines with how many each; then per kernel of the working tree's
build the VGPR count, scratch bytes and LDS bytes, with the other commit's where they differ.
Exit status 1 if any unit differs.
"""
import argparse
import concurrent.futures as cf
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = "ratatosk_amd/csrc"


def library_units():
    """the HIP translation units of the library: the hip/*.o among the prerequisites of $(LIB) in the working tree's Makefile"""
    with open(os.path.join(ROOT, CSRC, "Makefile")) as f:
        rule = next(ln for ln in f if ln.startswith("$(LIB):"))
    return re.findall(r"\bhip/(\w+)\.o\b", rule)


def make_var(csrc, name):
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", csrc, "--eval",
                          "print-var: ; @echo $(%s)" % name, "print-var"],
                         check=True, capture_output=True, text=True).stdout
    return out.split()


def assemble(tree, unit, out):
    csrc = os.path.join(tree, CSRC)
    cmd = make_var(csrc, "HIPCC") + make_var(csrc, "HIPFLAGS") + [
        "-I../../include", "--offload-device-only", "-S", "-o", out, "hip/%s.hip" % unit]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("%s: %s\n%s" % (tree, " ".join(cmd), r.stderr))
    return r.stderr


def normalised(path):
    with open(path) as f:
        return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", f.read()).splitlines()


def resources(lines):
    """kernel name -> (vgprs, scratch bytes, LDS bytes), from the amdhsa.kernels metadata"""
    res, cur = {}, {}
    for ln in lines:
        # a kernel's own keys are indented by four columns; those of its arguments (.name too) by more
        m = re.match(r"    \.(name|vgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)", ln)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "vgpr_count":  # the last of a kernel's keys (they are sorted)
            res[cur["name"]] = (int(cur["vgpr_count"]), int(cur["private_segment_fixed_size"]),
                                int(cur["group_segment_fixed_size"]))
            cur = {}
    return res


def functions(lines):
    """[(function, its lines)] in the order of the text.  A function begins at its `.type NAME,@function`; what stands in front of the first one is
    "(head)", the metadata behind the last one "(tail)".  The number of the function inside its local labels (.LBB12_3, .Lfunc_end12) is taken
    out, so that a function added or removed further up does not make every later one differ."""
    out, name, cur = [], "(head)", []
    for ln in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m or (name not in ("(head)", "(tail)") and re.match(r"\s*\.(amdgpu_metadata|type\s+\S+,@object)", ln)):
            out.append((name, cur))
            name, cur = (m.group(1) if m else "(tail)"), []
        cur.append(re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)\d+", r".\1", ln))
    out.append((name, cur))
    return out


def demangled(names):
    """mangled -> name without its parameter list (c++filt when there is one, else the mangled name)"""
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        r = names
    return {n: n if n.startswith("(") else re.sub(r"^(?:void |\(anonymous namespace\)::)*", "", d).split("(")[0] for n, d in zip(names, r)}  # "(head)", "(tail)" stay


def differing_functions(mine, theirs):
    """[(function, differing lines, lines here, lines there or None)] for the functions whose text is not the same on both sides"""
    fm, ft = functions(mine), dict(functions(theirs))
    out = []
    for name, a in fm:
        b = ft.pop(name, None)
        if b is None:
            out.append((name, len(a), len(a), None))
        elif a != b:
            if len(a) == len(b):
                nd = sum(x != y for x, y in zip(a, b))
            else:
                nd = sum(1 for d in difflib.unified_diff(b, a, n=0, lineterm="") if d[:1] in "+-" and d[:3] not in ("+++", "---"))
            out.append((name, nd, len(a), len(b)))
    return out, [(n, len(b)) for n, b in ft.items()]


def short_name(mangled):
    """k_regions of _Z9k_regionsPK9LaunchCtx...; None for a kernel that is not the project's (library templates)"""
    m = re.search(r"(\d+)(k_\w+)", mangled)
    if not m:
        return None
    digits = m.group(1)  # may begin with the end of what stands in front (_GLOBAL__N_1 10k_col_pack): the longest count that fits
    n = next((int(digits[i:]) for i in range(len(digits)) if int(digits[i:]) <= len(m.group(2))), len(m.group(2)))
    name = m.group(2)[:n]
    t = re.match(r"I([a-z])E", m.group(2)[n:])
    return name + ("<%s>" % {"m": "u64", "o": "u128"}.get(t.group(1), t.group(1)) if t else "")


def warning_lines(stderr):
    return [re.sub(r"^.*?(hip/[^:]+):\d+:\d+: ", r"\1: ", ln) for ln in stderr.splitlines() if "warning:" in ln]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("commit", nargs="?", default="HEAD^")
    ap.add_argument("--keep", metavar="DIR")
    a = ap.parse_args()
    tmp = None
    if a.keep:
        work = os.path.abspath(a.keep)
        os.makedirs(work, exist_ok=True)
    else:
        tmp = tempfile.TemporaryDirectory()
        work = tmp.name
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.commit], check=True,
                         capture_output=True, text=True).stdout.strip()
    other = os.path.join(work, "tree_" + sha)
    if not os.path.isdir(other):  # extracted under another name first: a tree that --keep reuses is a whole one
        part = other + ".part"
        os.makedirs(part)
        ar = subprocess.Popen(["git", "-C", ROOT, "archive", sha, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", part], stdin=ar.stdout, check=True)
        if ar.wait() != 0:
            sys.exit("git archive %s failed" % sha)
        os.rename(part, other)
    jobs = {}
    UNITS = library_units()
    only_here = [u for u in UNITS if not os.path.exists(os.path.join(other, CSRC, "hip", u + ".hip"))]
    with cf.ThreadPoolExecutor(max_workers=min(len(os.sched_getaffinity(0)), 2 * len(UNITS))) as ex:
        for u in UNITS:
            theirs = os.path.join(work, "%s_%s.s" % (u, sha))
            if u in only_here:
                open(theirs, "w").close()
            elif not os.path.exists(theirs):
                jobs[(u, "theirs")] = ex.submit(assemble, other, u, theirs)
            jobs[(u, "ours")] = ex.submit(assemble, ROOT, u, os.path.join(work, u + "_tree.s"))
    warnings = {k: f.result() for k, f in jobs.items()}
    print("device assembly of the working tree against %s" % sha)
    print("flags: %s -I../../include --offload-device-only -S" % " ".join(make_var(os.path.join(ROOT, CSRC), "HIPFLAGS")))
    differ = 0
    table, library = [], []
    for u in UNITS:
        mine = normalised(os.path.join(work, u + "_tree.s"))
        theirs = normalised(os.path.join(work, "%s_%s.s" % (u, sha)))
        same = mine == theirs
        differ += not same
        nd = sum(x != y for x, y in zip(mine, theirs)) + abs(len(mine) - len(theirs))
        print("  hip/%-22s %7d lines  %s" % (u + ".hip", len(mine),
                                              "identical" if same else "DIFFERS (%d lines, %d there)" % (nd, len(theirs))))
        if u in only_here:
            print("    (the other commit has no such unit)")
        elif not same:
            funcs, gone = differing_functions(mine, theirs)
            names = demangled([f[0] for f in funcs] + [g[0] for g in gone])
            print("    functions that differ (local labels compared without the function's number): %d" % (len(funcs) + len(gone)))
            for name, n, here, there in funcs:
                print("      %-44s %6d lines differ  (%d here, %s there)" % (names[name], n, here, "none" if there is None else there))
            for name, there in gone:
                print("      %-44s only there (%d lines)" % (names[name], there))
        # compiler warnings of this side that the other side does not show (known only when both were built in this call)
        if (u, "theirs") in warnings:
            known = set(warning_lines(warnings[(u, "theirs")]))
            new = [w for w in warning_lines(warnings[(u, "ours")]) if w not in known]
            print("    hipcc warnings: %d here, %d there, %d new" % (len(warning_lines(warnings[(u, "ours")])), len(known), len(new)))
            for w in new:
                print("      " + w)
        rm, rt = resources(mine), resources(theirs)
        other_kernels = [k for k in rm if not short_name(k)]
        for k in sorted(rm, key=lambda k: short_name(k) or ""):
            if short_name(k):
                table.append((u, short_name(k), rm[k], rt.get(k)))
        if other_kernels:
            library.append((u, len(other_kernels), sum(rm[k] != rt.get(k) for k in other_kernels)))
    print("\nkernels of the working tree's build (the other side's figures follow where they differ)")
    print("%-18s %-26s %6s %9s %7s" % ("unit", "kernel", "VGPRs", "scratch B", "LDS B"))
    for u, k, m, t in table:
        print("%-18s %-26s %6d %9d %7d%s" % (u, k, m[0], m[1], m[2], "" if m == t else "   there: %s" % (t,)))
    for u, n, nd in library:
        print("%-18s %d kernels of library templates: %s" % (u, n, "%d differ" % nd if nd else "all equal"))
    if tmp:
        tmp.cleanup()
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
