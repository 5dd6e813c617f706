#!/usr/bin/env python3
"""Do two revisions compile to the same gfx950 instruction text?  (dev aid for restructurings; runs without a GPU)

    python tools/same_text.py BASE [NEW] [--units a.hip b.hip ...] [--keep DIR] [--jobs N]

BASE and NEW are each a source tree (a checkout of this repository: its gym_pomdp_amd/csrc is compiled) or a directory of kept
`<unit>.s` files; NEW defaults to the working tree.  Every translation unit of the product library (_native.UNITS) is compiled
to device assembly with the library's own flags, split per mangled symbol, and compared as text after comments, directives and
label numbers are stripped.  Prints the number of symbols per unit and the names and lengths of those that differ; exits
non-zero if any differ or the symbol sets differ.  `--keep DIR` keeps what was compiled as DIR/base/<unit>.s and
DIR/new/<unit>.s (a kept directory can be BASE the next time).
"""
import argparse
import os
import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gym_pomdp_amd import _native  # noqa: E402
from tools.isa_mix import compile_asm, demangle, kernels_of  # noqa: E402

LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def text_of(lines):
    """A symbol's instructions and labels: no comments, no directives, labels renumbered in order of appearance."""
    seen, out = {}, []
    for line in lines:
        s = line.split(";", 1)[0].strip()
        if not s or (s.startswith(".") and not s.endswith(":")):
            continue
        out.append(LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), " ".join(s.split())))
    return out


def symbols(side, unit, keep, jobs_dir):
    """-> {mangled symbol: stripped text} of `unit` in `side` (a source tree or a directory of .s files)"""
    csrc = os.path.join(side, "gym_pomdp_amd", "csrc")
    if os.path.isdir(csrc):
        out = os.path.join(keep or jobs_dir, unit + ".s")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        compile_asm(os.path.join(csrc, unit), out, _native.HIPCC_FLAGS)
    else:
        out = os.path.join(side, unit + ".s")
    return {k: text_of(v) for k, v in kernels_of(open(out).read()).items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("base")
    ap.add_argument("new", nargs="?", default=REPO)
    ap.add_argument("--units", nargs="+", default=list(_native.UNITS))
    ap.add_argument("--keep")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=a.jobs) as ex:
        sides = [(a.base, "base"), (a.new, "new")]
        jobs = {(u, tag): ex.submit(symbols, side, u, a.keep and os.path.join(a.keep, tag), os.path.join(tmp, tag))
                for u in a.units for side, tag in sides}
        for u in a.units:
            old, new = jobs[u, "base"].result(), jobs[u, "new"].result()
            gone, come = sorted(set(old) - set(new)), sorted(set(new) - set(old))
            differ = [k for k in old if k in new and old[k] != new[k]]
            print("%-24s %4d symbols, %d differ, %d only in base, %d only in new" % (u, len(old), len(differ), len(gone), len(come)), flush=True)
            names = demangle(differ + gone + come) if differ or gone or come else {}
            for k in differ:
                print("    differs (%d -> %d lines): %s" % (len(old[k]), len(new[k]), names[k]))
            for k in gone:
                print("    only in base (%d lines): %s" % (len(old[k]), names[k]))
            for k in come:
                print("    only in new (%d lines): %s" % (len(new[k]), names[k]))
            bad += len(differ) + len(gone) + len(come)
    print("same text" if not bad else "%d symbols differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
