#!/usr/bin/env python3
"""Per-kernel fingerprint of the gfx950 code of the fused GraphSAGE tree step, for refactors
that must not change the generated code.

    python tools/kernel_isa.py TREE_A TREE_B [--units GLOB ...] [--out DIR]

For each tree the translation units ``euler_amd/csrc/hip/<GLOB>`` (default: ``sage_tree.hip``
and ``tree_*.hip``, whichever exist) are compiled device-only with the kernel flags of
``euler_amd/_build.py``.  Every kernel of the code objects' metadata gets one table row:

    symbol  unit  instructions  sha256[:16] of the normalised stream  vgpr agpr sgpr
    vgpr_spill sgpr_spill lds private kernarg

The normalised stream is the disassembly of the symbol's own bytes (its address and size from
the symbol table, so padding behind the last instruction is not part of it), one instruction
per line, without the address / encoding / branch-target comment.  Branch operands are
relative, so the same code at another address gives the same stream.  CPU only: nothing runs.

Exit status 0: every kernel of TREE_A is in exactly one unit of TREE_B with an equal row
(the unit column aside); 1 otherwise.  With ``--out DIR`` the two tables are written to
``DIR/<name of tree>.tsv`` (``--names A B`` sets the names).
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

META = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size"]
HEAD = ["symbol", "unit", "insts", "stream_sha256", "vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill",
        "lds", "private", "kernarg"]


def _tool(name):
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)


def _out(cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout


def compile_unit(tree, unit, arch, objdir):
    csrc = os.path.join(tree, "euler_amd", "csrc")
    co = os.path.join(objdir, unit + ".co")
    hipcc = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))
    # the kernel flags of euler_amd/_build.py build_hip()
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", f"--offload-arch={arch}", "-munsafe-fp-atomics",
           "-D__HIP_PLATFORM_AMD__=1", "-I" + csrc, "-Wno-unused-result"]
    cmd += os.environ.get("EULER_AMD_HIP_FLAGS", "").split()
    cmd += ["--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(csrc, "hip", unit), "-o", co]
    subprocess.run(cmd, check=True)
    return co


def kernel_meta(co):
    """{symbol: {key: int}} from the amdhsa.kernels list of the metadata note."""
    kernels, cur = {}, None
    for line in _out([_tool("llvm-readelf"), "--notes", co]).splitlines():
        m = re.match(r"^  (-| ) \.(\w+):\s*(\S*)", line)  # keys of a kernel entry, not of its .args
        if not m:
            continue
        if m.group(1) == "-":
            cur = {}
        if cur is None:
            continue
        if m.group(2) == "name":
            kernels[m.group(3)] = cur
        elif m.group(2) in META:
            cur[m.group(2)] = int(m.group(3))
    return kernels


def symbol_ranges(co):
    out = {}
    for line in _out([_tool("llvm-readelf"), "-sW", co]).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            out[f[7]] = (int(f[1], 16), int(f[2]))
    return out


def streams(co, ranges):
    """{symbol: [instruction text]} restricted to each symbol's own bytes."""
    spans = sorted((a, a + n, s) for s, (a, n) in ranges.items())
    out = {s: [] for s in ranges}
    k = 0
    for line in _out([_tool("llvm-objdump"), "-d", co]).splitlines():
        m = re.match(r"^\s+(\S.*?)\s*// ([0-9A-Fa-f]+):", line)
        if not m:
            continue
        addr = int(m.group(2), 16)
        while k < len(spans) and addr >= spans[k][1]:
            k += 1
        if k < len(spans) and spans[k][0] <= addr:
            out[spans[k][2]].append(re.sub(r"\s+", " ", m.group(1)))
    return out


def table(tree, units, arch):
    """[(row, ...)] sorted by symbol; a symbol found in two units gives two rows."""
    hdir = os.path.join(tree, "euler_amd", "csrc", "hip")
    names = sorted({os.path.basename(p) for g in units for p in glob.glob(os.path.join(hdir, g))})
    if not names:
        raise SystemExit(f"{tree}: no unit matches {units}")
    rows = []
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(max_workers=min(8, len(names))) as ex:
        for unit, co in zip(names, ex.map(lambda u: compile_unit(tree, u, arch, tmp), names)):
            meta = kernel_meta(co)
            st = streams(co, symbol_ranges(co))
            for sym, md in meta.items():
                text = "\n".join(st[sym])
                rows.append((sym, unit, len(st[sym]), hashlib.sha256(text.encode()).hexdigest()[:16]) +
                            tuple(md[k] for k in META))
    return sorted(rows)


def render(rows):
    return "".join("\t".join(str(x) for x in r) + "\n" for r in [tuple(HEAD)] + rows)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--units", nargs="+", default=["sage_tree.hip", "tree_*.hip"])
    ap.add_argument("--arch", default=os.environ.get("EULER_AMD_ARCH", "gfx950"))
    ap.add_argument("--out")
    ap.add_argument("--names", nargs=2, default=["a", "b"])
    args = ap.parse_args(argv)
    ta, tb = (table(t, args.units, args.arch) for t in (args.tree_a, args.tree_b))
    for name, t in zip(args.names, (ta, tb)):
        print(f"# {name}: {len(t)} kernels")
        sys.stdout.write(render(t))
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, name + ".tsv"), "w") as f:
                f.write(render(t))
    bad = 0
    for row in ta:
        hits = [r for r in tb if r[0] == row[0]]
        if len(hits) != 1:
            print(f"DIFF {row[0]}: in {len(hits)} units of {args.names[1]}")
            bad += 1
        elif hits[0][2:] != row[2:]:
            print(f"DIFF {row[0]}:\n  {args.names[0]}: {row[2:]}\n  {args.names[1]}: {hits[0][2:]}")
            bad += 1
    print(f"{len(ta) - bad} of {len(ta)} kernels of {args.names[0]} equal in {args.names[1]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
