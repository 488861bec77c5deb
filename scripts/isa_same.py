#!/usr/bin/env python3
"""Compare the gfx950 device assembly of csrc/*.hip files between a git revision and the tree.

    python scripts/isa_same.py [REV] nuts.hip potential_logreg.hip ...      (REV defaults to HEAD~1)

Both trees are compiled with the release flags of numpyro_amd/build.py plus
``-x hip --cuda-device-only -S``.  The output is split at function symbols (a kernel's text runs
from its label to its ``.Lfunc_end``, which encloses its ``.amdhsa_kernel`` descriptor: register
counts, scratch, LDS) and compared as text.  Lines with ``__hip_cuid_`` (a hash that differs between
any two compiles) are dropped, and so is the per-file function index in block labels
(``.LBB12_3``, ``BB12_3`` in comments, ``.Lfunc_end12``): it shifts when an earlier instantiation
goes away.  Exits non-zero if any function differs or is new; removed ones are only listed.
"""
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from numpyro_amd.build import COMMON_FLAGS, FILE_FLAGS, HIPCC  # noqa: E402

LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):\s+; @")
LOCAL = re.compile(r"(\.L(?:BB|JTI|func_begin|func_end)|\bBB)\d+")


def functions(root, name, out):
    """{symbol: normalised text} of one file compiled in the tree at ``root``."""
    flags = [f.replace(ROOT, root) if f.startswith("-I") else f for f in COMMON_FLAGS]
    src = os.path.join(root, "numpyro_amd", "csrc", name)
    cmd = [HIPCC, *flags, *FILE_FLAGS.get(name, ()), "-x", "hip", "--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    funcs, sym = {}, None
    with open(out) as f:
        for line in f:
            if "__hip_cuid_" in line:
                continue
            m = LABEL.match(line)
            if m:
                sym = m.group(1)
                funcs[sym] = []
            if sym is not None:
                funcs[sym].append(LOCAL.sub(r"\1", line))
                if line.startswith(".Lfunc_end"):
                    sym = None
    return {k: "".join(v) for k, v in funcs.items()}


def demangle(syms):
    if not syms:
        return []
    r = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True)
    return r.stdout.splitlines() if r.returncode == 0 else list(syms)


def main(argv):
    rev = "HEAD~1"
    if argv and not argv[0].endswith(".hip"):
        rev, argv = argv[0], argv[1:]
    if not argv:
        sys.exit(__doc__)
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old_root = os.path.join(tmp, "old")
        os.makedirs(old_root)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", old_root], input=tar, check=True)
        with cf.ThreadPoolExecutor(max_workers=8) as ex:
            jobs = {(n, side): ex.submit(functions, root, n, os.path.join(tmp, f"{side}_{n}.s"))
                    for n in argv for side, root in (("old", old_root), ("new", ROOT))}
        for n in argv:
            old, new = jobs[n, "old"].result(), jobs[n, "new"].result()
            removed = sorted(set(old) - set(new))
            added = sorted(set(new) - set(old))
            differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
            print(f"{n}: {len(old)} functions in {rev}, {len(new)} now: "
                  f"{len(removed)} removed, {len(added)} new, {len(differ)} differ")
            for title, syms in (("only in " + rev, removed), ("only in the tree", added), ("differ", differ)):
                for s in demangle(syms):
                    print(f"  {title}: {s}")
            bad += len(added) + len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
