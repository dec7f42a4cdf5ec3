"""Compare the gfx950 kernel bodies of two source trees as text: the proof of a refactor that is meant to change no kernel.

    python tools/kernel_bodies.py --a PARENT_TREE a.hip [b.hip ...] --b THIS_TREE c.hip [d.hip ...] [--resources REGEX] [--markdown]

PARENT_TREE and THIS_TREE are repository roots (e.g. a `git worktree` of the parent commit and the working tree); the files are
names in their cubesat-apds_amd/csrc. Every file is compiled with the CXXFLAGS of that tree's csrc/Makefile plus
`-S --cuda-device-only -Rpass-analysis=kernel-resource-usage`, at most 16 at a time. The assembly is cut into kernels by label
(the symbols that carry an `.amdhsa_kernel` descriptor); of a kernel's lines between its label and its `.Lfunc_end`, comments,
directives and blank lines are dropped and the `.LBB` labels renumbered in order of appearance. Per kernel symbol the report
says identical / differs / gone / new, with the count of instructions and labels. `--resources` adds, for the kernels whose
demangled name matches, the resource-usage remarks of either side. The script compares text and nothing else; it exits 1
unless both sides hold the same symbols with identical bodies (and equal remarks).
"""
import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
REMARK_KEYS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]


def makefile_flags(csrc):
    for line in open(os.path.join(csrc, "Makefile")):
        if line.startswith("CXXFLAGS"):
            return line.split("=", 1)[1].replace("$(ARCH)", "gfx950").replace("$(EXTRA_CXXFLAGS)", "").split()
    raise SystemExit(f"no CXXFLAGS in {csrc}/Makefile")


def compile_one(job):
    csrc, name, out = job
    # a fixed -cuid: the suffix of externalised internal-linkage symbols must not depend on where the tree lies
    cmd = [HIPCC] + makefile_flags(csrc) + ["-S", "--cuda-device-only", "-cuid=kernelbodies", "-Rpass-analysis=kernel-resource-usage", name, "-o", out]
    r = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        raise SystemExit(f"{' '.join(cmd)}\n{r.stderr}")
    return out, r.stderr


def kernel_bodies(asm_path):
    lines = open(asm_path).read().split("\n")
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    bodies, cur, body = {}, None, None
    for line in lines:
        m = re.match(r"^([A-Za-z_$.][\w$.]*):", line)
        if m and m.group(1) in kernels and cur is None:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            bodies[cur] = body
            cur = None
            continue
        s = line.split(";", 1)[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        body.append(s)
    out = {}
    for k, b in bodies.items():
        names = {}
        for s in b:
            for lab in re.findall(r"\.LBB\d+_\d+", s):
                names.setdefault(lab, f".L{len(names)}")
        out[k] = [re.sub(r"\.LBB\d+_\d+", lambda m: names[m.group(0)], s) for s in b]
    return out


def kernel_remarks(stderr):
    """{kernel symbol: {key: value}} from the kernel-resource-usage remarks"""
    out, cur = {}, None
    for line in stderr.split("\n"):
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}(.+?): (\S+)\s*\[-Rpass-analysis", line) or re.search(r"remark: .*?\s{2,}(.+?): (\S+)\s*$", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def side(root, files, tmp, tag, pool):
    csrc = os.path.join(os.path.abspath(root), "cubesat-apds_amd", "csrc")
    jobs = [(csrc, f, os.path.join(tmp, f"{tag}_{f}.s")) for f in files]
    bodies, remarks, where = {}, {}, {}
    for (out, err), (_, f, _) in zip(pool.map(compile_one, jobs), jobs):
        b = kernel_bodies(out)
        for k in b:
            if k in bodies:
                raise SystemExit(f"{k} is defined twice on side {tag}")
            where[k] = f
        bodies.update(b)
        remarks.update(kernel_remarks(err))
    return bodies, remarks, where


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        got = subprocess.run([filt], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
        return dict(zip(names, got))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    """the demangled name without its return type and parameter list"""
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)", "{anonymous}")
    depth = 0
    for i, ch in enumerate(name):   # the first '(' outside the template arguments opens the parameter list
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", nargs="+", required=True, metavar=("TREE", "FILE"))
    ap.add_argument("--b", nargs="+", required=True, metavar=("TREE", "FILE"))
    ap.add_argument("--resources", default=None, help="regex on demangled kernel names: list their resource remarks")
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--keep", default=None, help="keep the assembly in this directory")
    args = ap.parse_args()
    tmp = args.keep or tempfile.mkdtemp(prefix="kernel_bodies_")
    os.makedirs(tmp, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(max_workers=16) as pool:
        fa = pool.submit(side, args.a[0], args.a[1:], tmp, "a", pool)
        fb = pool.submit(side, args.b[0], args.b[1:], tmp, "b", pool)
        (ba, ra, wa), (bb, rb, wb) = fa.result(), fb.result()
    names = demangle(sorted(set(ba) | set(bb)))
    count = {"identical": 0, "differs": 0, "gone": 0, "new": 0}
    rows = []
    for k in sorted(names, key=lambda k: (wb.get(k, wa.get(k)), names[k])):
        state = "gone" if k not in bb else "new" if k not in ba else "identical" if ba[k] == bb[k] else "differs"
        count[state] += 1
        n = len(bb[k]) if k in bb else len(ba[k])
        if state == "differs":
            n = f"{len(ba[k])} -> {len(bb[k])}"
        rows.append((short(names[k]), wa.get(k, "-"), wb.get(k, "-"), n, state))
    sep = " | " if args.markdown else "  "
    if args.markdown:
        print("| kernel | file at A | file at B | instructions and labels | body |\n|---|---|---|---|---|")
    for r in rows:
        line = sep.join(f"`{c}`" if args.markdown and i == 0 else str(c) for i, c in enumerate(r))
        print(f"| {line} |" if args.markdown else line)
    unequal = 0
    if args.resources:
        print()
        if args.markdown:
            print("| kernel | " + " | ".join(REMARK_KEYS) + " | against A |\n|---|" + "---|" * (len(REMARK_KEYS) + 1))
        for k in sorted(names, key=lambda k: names[k]):
            if not re.search(args.resources, names[k]):
                continue
            va, vb = ra.get(k, {}), rb.get(k, {})
            same = va == vb and bool(vb)
            unequal += 0 if same else 1
            cells = [vb.get(key, "?") for key in REMARK_KEYS]
            verdict = "equal" if same else "A: " + ", ".join(va.get(key, "?") for key in REMARK_KEYS)
            line = sep.join([f"`{short(names[k])}`" if args.markdown else short(names[k])] + cells + [verdict])
            print(f"| {line} |" if args.markdown else line)
    all_unequal = sum(1 for k in names if ra.get(k) != rb.get(k))
    print(f"\n{len(ba)} kernels at A, {len(bb)} at B: {count['identical']} identical, {count['differs']} differ, {count['gone']} gone, {count['new']} new; "
          f"resource remarks of {len(names) - all_unequal} of {len(names)} equal")
    if not args.keep:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0 if count["identical"] == len(names) and not all_unequal and not unequal else 1


if __name__ == "__main__":
    sys.exit(main())
