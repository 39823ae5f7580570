#!/usr/bin/env python3
"""Compare the gfx950 code of every kernel between two trees of this repository (a parent checkout and a change).

    python tools/kernel_isa_diff.py PARENT_ROOT CHILD_ROOT [--jobs N] [--times]

Every unit in each tree's fp8q/build.py SOURCES is compiled with build.py's flags plus `--cuda-device-only -S`.  A kernel
is its body (label to function end) and its .amdhsa_kernel descriptor block, keyed by unit and demangled name; a kernel
that left a unit is looked up in the units only the child has (a file split).  Function-local label numbers, which count
the functions in front of a kernel in its file, are the only thing normalised.  Prints one line per unit, every kernel
that differs with its VGPR / LDS / scratch numbers side by side, and with --times the device-only compile time per unit.
Needs no GPU.
"""
import argparse
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
import time


def load_build(root):
    path = os.path.join(root, "fp8-quantization_amd", "fp8q", "build.py")
    spec = importlib.util.spec_from_file_location("fp8q_build_" + str(abs(hash(root))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_unit(job):
    hipcc, cflags, csrc, unit, out = job
    t0 = time.time()
    subprocess.check_call([hipcc] + cflags + ["--cuda-device-only", "-S", os.path.join(csrc, unit), "-o", out], cwd=csrc,
                          stderr=subprocess.DEVNULL)
    return unit, out, time.time() - t0


LABEL = re.compile(r"\.L(BB|func_end|func_begin|tmp)(\d+)")


def normalise(lines):
    return [LABEL.sub(lambda m: ".L" + m.group(1) + "#", ln).rstrip() for ln in lines]


def parse(path, demangle):
    """{demangled kernel name: (body lines, descriptor lines)} and the rest of the file (device functions, tables)."""
    lines = open(path).read().split("\n")
    kernels = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    names = dict(zip(kernels, demangle(kernels)))
    out = {}
    rest = []
    i = 0
    cur = None
    while i < len(lines):
        ln = lines[i]
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            j = i
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            out.setdefault(m.group(1), [None, None])[1] = normalise(lines[i:j + 1])
            i = j + 1
            continue
        lab = re.match(r"(\S+):\s*(;.*)?$", ln)      # (the compiler may print "; @name" behind a function's label)
        if lab and lab.group(1) in names and cur is None:
            cur = lab.group(1)
            j = i
            while not re.match(r"\.Lfunc_end\d+:", lines[j]):
                j += 1
            out.setdefault(cur, [None, None])[0] = normalise(lines[i:j])
            for d in range(i, j):      # (the descriptor block may sit in front of the function's end label)
                if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(cur) + r"\s*$", lines[d]):
                    e = d
                    while ".end_amdhsa_kernel" not in lines[e]:
                        e += 1
                    out[cur][1] = normalise(lines[d:e + 1])
            i = j + 1
            cur = None
            continue
        if "__hip_cuid" not in ln and not ln.lstrip().startswith((".file", ".ident")):
            rest.append(ln)
        i += 1
    lost = [names[k] for k, v in out.items() if v[0] is None or v[1] is None]
    if lost:      # a kernel whose body went unrecognised would be compared by its descriptor alone
        sys.exit("%s: no body or no descriptor found for %d kernels, first %s" % (path, len(lost), lost[0]))
    return {names[k]: tuple(v) for k, v in out.items()}, normalise(rest)


def field(desc, key):
    for ln in desc:
        m = re.match(r"\s*\.amdhsa_%s\s+(\S+)" % key, ln)
        if m:
            return m.group(1)
    return "?"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("child")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--times", action="store_true")
    a = ap.parse_args()
    trees = {}
    with tempfile.TemporaryDirectory(prefix="isa_diff_") as tmp:
        jobs = []
        for tag, root in (("parent", a.parent), ("child", a.child)):
            b = load_build(os.path.abspath(root))
            trees[tag] = b.SOURCES
            jobs += [(b._hipcc(), b.CFLAGS, b.CSRC, u, os.path.join(tmp, tag + "_" + u + ".s")) for u in b.SOURCES]
        with concurrent.futures.ThreadPoolExecutor(max_workers=a.jobs) as pool:
            done = list(pool.map(compile_unit, jobs))
        cxxfilt = os.path.join(os.path.dirname(jobs[0][0]), "..", "llvm", "bin", "llvm-cxxfilt")

        def demangle(names):
            if not names:
                return []
            return subprocess.run([cxxfilt if os.path.exists(cxxfilt) else "c++filt"], input="\n".join(names), text=True,
                                  capture_output=True, check=True).stdout.split("\n")[:len(names)]

        asm = {"parent": {}, "child": {}}
        secs = {"parent": {}, "child": {}}
        for (hipcc, cflags, csrc, unit, out), (_, _, dt) in zip(jobs, done):
            tag = os.path.basename(out).split("_", 1)[0]
            asm[tag][unit] = parse(out, demangle)
            secs[tag][unit] = dt
    new_units = [u for u in trees["child"] if u not in trees["parent"]]
    pool_new = {}
    for u in new_units:
        for name, kd in asm["child"][u][0].items():
            pool_new[name] = (u, kd)
    bad = 0
    used_new = set()
    print("unit                     kernels  identical  moved-to-new-units  rest-of-file")
    for u in trees["parent"]:
        pk = asm["parent"][u][0]
        ck = asm["child"].get(u, ({}, []))[0]
        same = moved = 0
        for name, kd in sorted(pk.items()):
            where, other = (u, ck[name]) if name in ck else pool_new.get(name, (None, None))
            if where is None:
                print("  MISSING in child: %s" % name)
                bad += 1
                continue
            if where != u:
                moved += 1
                used_new.add(name)
            if other == kd:
                same += 1
                continue
            bad += 1
            print("  DIFFERS: %s (%s -> %s)" % (name, u, where))
            for key in ("next_free_vgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size"):
                print("      %-28s parent %-8s child %s" % (key, field(kd[1], key), field(other[1], key)))
        extra = [n for n in ck if n not in pk]
        for n in extra:
            print("  EXTRA in child unit %s: %s" % (u, n))
        bad += len(extra)
        rest = "-" if u not in asm["child"] else "(split)" if moved else ("same" if asm["child"][u][1] == asm["parent"][u][1] else "DIFFERS")
        print("%-24s %7d %10d %19d  %s" % (u, len(pk), same, moved, rest))
    for u in new_units:
        ks = asm["child"][u][0]
        stray = [n for n in ks if n not in used_new]
        for n in stray:
            print("  EXTRA in new unit %s: %s" % (u, n))
        bad += len(stray)
        print("%-24s %7d kernels, all from the parent: %s" % (u + " (new)", len(ks), "yes" if not stray else "NO"))
    print("total kernels: parent %d, child %d" % (sum(len(v[0]) for v in asm["parent"].values()),
                                                  sum(len(v[0]) for v in asm["child"].values())))
    if a.times:
        print("device-only compile seconds (%d jobs in parallel):" % a.jobs)
        for tag in ("parent", "child"):
            print("  %s: %s" % (tag, ", ".join("%s %.1f" % (u, secs[tag][u]) for u in trees[tag])))
    print("RESULT: %s" % ("every kernel identical" if bad == 0 else "%d kernels differ, are missing or are extra" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
