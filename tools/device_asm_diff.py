#!/usr/bin/env python3
"""Compare the gfx950 device assembly of every translation unit between two trees.

    python tools/device_asm_diff.py [OLD [NEW]]        (default: HEAD~1 HEAD)

OLD and NEW are git revisions, or directories that hold a tree (``.`` is the working tree).  Each tree's
``adsorbdiff_amd/csrc`` and ``include`` are exported to a temporary directory and every entry of that tree's
``build.SOURCES`` is compiled with its ``build.FLAGS`` + ``build.EXTRA_FLAGS`` + ``--cuda-device-only -S``.  The
compiler runs inside ``csrc`` on the relative file name and without a compilation-unit id (a hash of the absolute
path), so no path reaches the output.  One line per unit:
``identical``, or ``differs`` and the kernels whose text differs.  Files are compared as bytes; nothing is looked
for in them.  A refactor that only moves always-inline helpers must report ``identical`` everywhere: that proves
results and kernel speed untouched without a GPU.  Exit status 1 if any unit differs.
"""
from __future__ import annotations

import argparse
import io
import re
import runpy
import shutil
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
KEEP = ("adsorbdiff_amd/csrc", "adsorbdiff_amd/build.py", "include")
JOBS = 16


def export(tree: str, dst: Path) -> None:
    """Put KEEP of a revision (or of a directory) under dst."""
    if Path(tree).is_dir():
        for k in KEEP:
            src = Path(tree) / k
            if src.is_dir():
                shutil.copytree(src, dst / k, ignore=shutil.ignore_patterns("build"))
            else:
                (dst / k).parent.mkdir(parents=True, exist_ok=True)
                shutil.copy(src, dst / k)
        return
    tar = subprocess.run(["git", "-C", str(REPO), "archive", tree, "--", *KEEP], check=True, capture_output=True).stdout
    tarfile.open(fileobj=io.BytesIO(tar)).extractall(dst, filter="data")


def compile_tree(root: Path, out: Path) -> dict[str, bytes]:
    """Device assembly of every unit of the tree at root, by unit name."""
    b = runpy.run_path(str(root / "adsorbdiff_amd" / "build.py"))
    cc, csrc = b["_hipcc"](), root / "adsorbdiff_amd" / "csrc"
    out.mkdir(parents=True, exist_ok=True)

    def one(s: str) -> tuple[str, bytes]:
        asm = out / (s + ".s")
        res = subprocess.run([cc, *b["FLAGS"], *b["EXTRA_FLAGS"].get(s, []), "--cuda-device-only", "-S",
                              "-fuse-cuid=none", s, "-o", str(asm)], cwd=csrc, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"hipcc failed on {s}:\n{res.stdout}{res.stderr}")
        return s, asm.read_bytes()

    with ThreadPoolExecutor(max_workers=JOBS) as ex:
        return dict(ex.map(one, b["SOURCES"]))


def functions(asm: bytes) -> dict[str, bytes]:
    """Split one assembly file into its functions: from each `.type NAME,@function` to the next."""
    parts = re.split(rb"^\s*\.type\s+([^\s,]+),@function\s*$", asm, flags=re.M)
    return dict(zip(parts[1::2], parts[2::2]))


def changed(a: bytes, b: bytes) -> list[str]:
    fa, fb = functions(a), functions(b)
    names = sorted(n for n in fa.keys() | fb.keys() if fa.get(n) != fb.get(n))
    return [n.decode() for n in names] or ["(outside any function)"]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old", nargs="?", default="HEAD~1")
    ap.add_argument("new", nargs="?", default="HEAD")
    ap.add_argument("--keep", metavar="DIR", help="leave the exported trees and the assembly files in DIR")
    args = ap.parse_args()
    tmp = Path(args.keep) if args.keep else Path(tempfile.mkdtemp(prefix="device_asm_diff_"))
    try:
        asm = []
        for side, tree in (("old", args.old), ("new", args.new)):
            export(tree, tmp / side)
            asm.append(compile_tree(tmp / side, tmp / (side + "_asm")))
        old, new = asm
        differs = 0
        for unit in sorted(old.keys() | new.keys()):
            if unit not in old or unit not in new:
                print(f"{unit:22s} differs  (only in {'new' if unit in new else 'old'})")
            elif old[unit] == new[unit]:
                print(f"{unit:22s} identical")
                continue
            else:
                print(f"{unit:22s} differs  " + " ".join(changed(old[unit], new[unit])))
            differs += 1
        print(f"{len(old.keys() | new.keys())} units, {differs} differ")
        return 1 if differs else 0
    finally:
        if not args.keep:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
