#!/usr/bin/env python3
"""Vector instructions beside the MFMAs in the tile loop of the matrix-core likelihood kernel.

On gfx950 fp64 MFMA and every vector instruction share one pipe: next to the 40 MFMAs of a tile only the
COUNT of the other vector instructions matters.  This tool compiles csrc/gh_loglik_mfma.hip for gfx950 exactly as
build.py does (device side only, to assembly; ~3 min), finds the tile loop of the named instantiations -- the basic
blocks with the most MFMAs: one tile of MFMAs and the epilogue of the tile before it each, two of them per iteration in
fp64 -- and prints their vector instructions by opcode, the s_nop, and the kernel's registers.

    python tools/epilogue_isa.py                       # every fp64 instantiation with 20 k-steps (D <= 40)
    python tools/epilogue_isa.py double,20,8,false,false,true float,20,8,false     # T,KS,MP,MULTI,FE,BND
    python tools/epilogue_isa.py --asm listing.s ...   # a listing made earlier (--keep writes one)
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-recognition_amd")


def listing(path_out):
    spec = importlib.util.spec_from_file_location("gmmhmm_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    src = "gh_loglik_mfma.hip"
    flags = [f for f in b.FLAGS if f != "-fPIC"]
    cmd = [b.HIPCC] + flags + b.EXTRA.get(src, []) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, src), "-o", path_out]
    print(" ".join(cmd), file=sys.stderr, flush=True)
    subprocess.run(cmd, check=True)


def mangled(inst):
    """double,20,8,false,false -> the template-argument part of the mangled name"""
    out = ""
    for a in inst.split(","):
        a = a.strip()
        out += {"double": "d", "float": "f"}.get(a) or ("Lb%dE" % (a == "true") if a in ("true", "false") else "Li%dE" % int(a))
    return "loglik_mfma_kernelI" + out + "E"


def kernels(asm):
    for m in re.finditer(r"\n(_Z\w*loglik_mfma_kernel\w*):[^\n]*\n", asm):
        end = asm.index(".end_amdhsa_kernel", m.end())
        yield m.group(1), asm[m.end():end]


def tile_blocks(body):
    """The basic blocks of the innermost loop with the most MFMAs, in program order: one tile of MFMAs each, with the
    epilogue of the tile before (the flush test between two tiles ends a block, so the two tiles of an fp64 iteration are
    two blocks; the first and the last tiles of a frame block sit outside the loop and are not counted)."""
    blocks = []
    for blk in re.split(r"\n(?=\.LBB\d+_\d+:|; %bb\.\d+:)", body):    # (a block that is only fallen into has no label)
        lines = blk.split("\n")
        depth = re.search(r"Depth=(\d+)", lines[0]) if lines[0].startswith((".LBB", "; %bb.")) else None
        ins = [l.strip() for l in lines if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        blocks.append((sum(x.startswith("v_mfma") for x in ins), int(depth.group(1)) if depth else 0, ins))
    most = max(n for n, _, _ in blocks)
    deepest = max(d for n, d, _ in blocks if n == most)
    return [ins for n, d, ins in blocks if n == most and d == deepest], most


def report(name, body):
    blocks, n_mfma = tile_blocks(body)
    reg = {k: re.search(re.escape(k) + r"\s+(\S+)", body).group(1) for k in (".amdhsa_next_free_vgpr", ".amdhsa_accum_offset")
           if re.search(re.escape(k) + r"\s+(\S+)", body)}
    print("%s  %s" % (name, reg))
    total = 0
    for k, ins in enumerate(blocks):
        ops = Counter(x.split()[0] for x in ins)
        valu = {o: v for o, v in ops.items() if o.startswith("v_") and not o.startswith("v_mfma")}
        if k == 0:
            total = sum(valu.values())
        print("  tile block %d of %d: %d MFMAs, %d vector instructions, %d s_nop, %d LDS, %d global, %d scalar"
              % (k + 1, len(blocks), n_mfma, sum(valu.values()), ops.get("s_nop", 0), sum(v for o, v in ops.items() if o.startswith("ds_")),
                 sum(v for o, v in ops.items() if o.startswith("global_")), sum(v for o, v in ops.items() if o.startswith("s_") and o != "s_nop")))
        print("    " + ", ".join("%s %d" % kv for kv in sorted(valu.items(), key=lambda kv: (-kv[1], kv[0]))))
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("inst", nargs="*", help="template arguments T,KS,MP,MULTI[,FE[,BND]]; default: every fp64 instantiation with KS = 20")
    ap.add_argument("--asm", help="read this listing instead of compiling")
    ap.add_argument("--keep", help="write the listing here")
    a = ap.parse_args()
    if a.asm:
        asm = open(a.asm).read()
    else:
        path = a.keep or os.path.join(tempfile.mkdtemp(prefix="epilogue_isa_"), "gh_loglik_mfma.s")
        listing(path)
        asm = open(path).read()
    found = dict(kernels(asm))
    if a.inst:
        want = [mangled(i) for i in a.inst]
        names = [n for w in want for n in found if w in n]
        if len(names) < len(want):
            sys.exit("not in the listing: %s" % [w for w in want if not any(w in n for n in found)])
    else:
        names = sorted(n for n in found if "loglik_mfma_kernelIdLi20E" in n)
    for n in names:
        report(n, found[n])


if __name__ == "__main__":
    main()
