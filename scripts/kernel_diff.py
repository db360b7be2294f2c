#!/usr/bin/env python3
"""Compare the gfx950 machine code of every kernel of csrc/*.hip files between two
git revisions -- the check a refactor owes: the kernels it keeps compile to the same
instruction stream.

    python scripts/kernel_diff.py [OLD [NEW]] conv_gemm.hip conv3_halo.hip
    python scripts/kernel_diff.py HEAD . conv_wgrad.hip wgrad3_halo.hip \\
        --rename 'wgrad_kernelI(\\w+?)Li1EEEv=wgrad_kernelI\\1EEv' --rename 'wgrad3_halo_kernelIf=wgrad3_halo_kernelI'
    python scripts/kernel_diff.py HEAD . --pool pointwise.hip loss.hip optim.hip

OLD / NEW default to HEAD~1 / HEAD; `.` is the working tree.  Each file is compiled
device-only to assembly for both revisions (in a temporary directory), each kernel
is cut at its label ... .Lfunc_end, comments and directives are dropped, the function's
own symbol and the function number of its .LBB<n>_<m> labels are replaced, and the
instruction streams are compared per (mangled) name.  --rename 'REGEX=REPL' rewrites
the OLD names first, for kernels whose template parameter list changed.  With --pool the
kernels of all the files named are pooled per revision and compared by name (a file may
exist in one revision only): for kernels that moved between files; kernels in anonymous
namespaces have the same mangled name in every file.

Prints, per file (per pool), `identical a/b` (b = kernels present on both sides), then one line
per added, removed or differing kernel.  Exit status 1 if any kernel differs.
It compares only; it looks at nothing about which instructions appear.
"""
import argparse
import concurrent.futures as cf
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("vub_image_denoising_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-w"]


def checkout(rev, dst):
    """The sources of `rev` (csrc and the public header) under dst."""
    if rev == ".":
        for sub in (CSRC, "include"):
            shutil.copytree(os.path.join(REPO, sub), os.path.join(dst, sub),
                            ignore=shutil.ignore_patterns("*.o", "*.so", "*.s"))
        return
    tar = subprocess.run(["git", "-C", REPO, "archive", rev, CSRC, "include"], check=True, stdout=subprocess.PIPE)
    subprocess.run(["tar", "-x", "-C", dst], input=tar.stdout, check=True)


def compile_asm(root, name):
    out = os.path.join(root, name + ".s")
    src = os.path.join(root, CSRC, name)
    if not os.path.exists(src):
        return None
    subprocess.run([HIPCC, *FLAGS, src, "-o", out], check=True)
    return out


_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
_LBB = re.compile(r"\.LBB\d+_(\d+)")


def functions(path):
    """name -> normalised instruction lines of every kernel of an assembly file."""
    funcs, name, body = {}, None, None
    types, kernels = set(), set()
    for raw in open(path):
        line = raw.split(";", 1)[0].rstrip()
        s = line.strip()
        if not s:
            continue
        if s.startswith(".type") and s.endswith("@function"):
            types.add(s.split()[1].split(",")[0])
            continue
        if s.startswith(".amdhsa_kernel "):
            kernels.add(s.split()[1])
            continue
        if name is None:
            m = _LABEL.match(s)
            if m and m.group(1) in types:
                name, body = m.group(1), []
            continue
        if s.startswith(".Lfunc_end"):
            funcs[name] = body
            name = None
            continue
        if s.startswith(".") and not s.startswith(".LBB"):
            continue                        # directive
        body.append(_LBB.sub(r".LBB_\1", " ".join(s.split())).replace(name, "@self"))
    return {k: v for k, v in funcs.items() if k in kernels}   # (not the device functions left un-inlined)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("revs_and_files", nargs="+", metavar="[OLD [NEW]] FILE.hip ...")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--pool", action="store_true", help="pool the kernels of all files per revision")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_intermixed_args()
    files = [os.path.basename(f) for f in a.revs_and_files if f.endswith(".hip")]
    revs = [r for r in a.revs_and_files if not r.endswith(".hip")]
    if not files or len(revs) > 2:
        ap.error("give at most two revisions and at least one csrc/*.hip file")
    old, new = {0: ("HEAD~1", "HEAD"), 1: (revs + ["HEAD"])[:2], 2: revs}[len(revs)]
    renames = [(re.compile(r.split("=", 1)[0]), r.split("=", 1)[1]) for r in a.rename]

    differs = 0
    with tempfile.TemporaryDirectory(prefix="kernel_diff_") as tmp:
        roots = {}
        for side, rev in (("old", old), ("new", new)):
            roots[side] = os.path.join(tmp, side)
            os.makedirs(roots[side])
            checkout(rev, roots[side])
        with cf.ThreadPoolExecutor(a.jobs) as pool:
            asm = {(side, f): pool.submit(compile_asm, roots[side], f) for side in roots for f in files}
            def pooled(which, names):
                out = {}
                for f in names:
                    path = asm[(which, f)].result()
                    out.update(functions(path) if path else {})
                return out
            for f, names in ([("pool", files)] if a.pool else [(f, [f]) for f in files]):
                fo, fn = pooled("old", names), pooled("new", names)
                for rx, repl in renames:
                    fo = {rx.sub(repl, k): v for k, v in fo.items()}
                both = sorted(set(fo) & set(fn))
                diff = [k for k in both if fo[k] != fn[k]]
                differs += len(diff)
                print(f"{f}: identical {len(both) - len(diff)}/{len(both)}  ({old}: {len(fo)}, {new}: {len(fn)} kernels)")
                for k in sorted(set(fn) - set(fo)):
                    print(f"  added    {k}")
                for k in sorted(set(fo) - set(fn)):
                    print(f"  removed  {k}")
                for k in diff:
                    print(f"  differs  {k}  ({len(fo[k])} -> {len(fn[k])} lines)")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
