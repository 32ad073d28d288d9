#!/usr/bin/env python3
"""Do two likelihood waves and one decode wave of the headline step fit a SIMD's register file together?

A gfx950 SIMD has 512 unified registers per lane.  While bench.py's headline step runs, two waves of
loglik_mfma_kernel<double,20,8,false,false,true> (the log-sum-exp against the pack-time bound) share every SIMD and the other lane's viterbi_chain_lanes_kernel<double,5,
false,false,false,LANE_PF> (the shallow-ring "beside" form of the lane = chain decode) runs underneath.  A decode wave that does not fit beside two likelihood
waves can only start in the registers of a likelihood wave that has retired, and then keeps the next likelihood wave out
until it ends.  With alloc(k) = next_free_vgpr (ArchVGPRs + AGPRs) rounded up to the granule of 8 the condition is

    2 * alloc(likelihood) + alloc(decode) <= 512.

This tool compiles csrc/gh_loglik_mfma.hip and csrc/gh_viterbi_chain.hip for gfx950 exactly as build.py does (device
side only, to assembly; ~4 min), prints next_free_vgpr, ArchVGPRs, AGPRs, the allocation, LDS and scratch of the two
instantiations, the left side of the condition, and the s_waitcnt vmcnt(n) of the decode kernel's column loops (the
loop without guards has to wait on a count, not on vmcnt(0): DESIGN 4.2).  Exit status 1 when the sum exceeds 512 or
either kernel has scratch.  It reads register / LDS metadata and opcodes only.

    python tools/headline_registers.py
    python tools/headline_registers.py --asm-loglik a.s --asm-chain b.s     # listings made earlier (--keep DIR writes them)
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-recognition_amd")
SIMD_REGISTERS = 512
GRANULE = 8
LOGLIK = ("gh_loglik_mfma.hip", "loglik_mfma_kernelIdLi20ELi8ELb0ELb0ELb1EE")     # T, KS, MP, MULTI, FE, BND: the default fp64 form
DECODE = ("gh_viterbi_chain.hip", "viterbi_chain_lanes_kernelIdLi5ELb0ELb0ELb0ELi")     # + ring depth: the shallowest


def listing(src, path_out):
    spec = importlib.util.spec_from_file_location("gmmhmm_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    flags = [f for f in b.FLAGS if f != "-fPIC"]
    cmd = [b.HIPCC] + flags + b.EXTRA.get(src, []) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, src), "-o", path_out]
    print(" ".join(cmd), file=sys.stderr, flush=True)
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return path_out


def kernel(asm, tag):
    """(name, body up to .end_amdhsa_kernel) of the kernel whose mangled name holds `tag`; of several (the decode kernel's
    ring depths: the last template argument) the one with the smallest last argument"""
    found = list(re.finditer(r"\n(_Z\w*" + re.escape(tag) + r"(\d*)\w*):[^\n]*\n", asm))
    if not found:
        sys.exit("not in the listing: " + tag)
    m = min(found, key=lambda f: int(f.group(2) or 0))
    body = asm[m.end():asm.index(".end_amdhsa_kernel", m.end())]
    for key in ("num_vgpr", "num_agpr"):      # (the compiler's per-function summary follows the descriptor)
        s = re.search(r"\.set " + re.escape(m.group(1)) + r"\." + key + r", (\d+)", asm)
        body += "\n; %s: %s" % (key, s.group(1) if s else "0")
    return m.group(1), body


def meta(body):
    def num(key, default=None):
        m = re.search(re.escape(key) + r":?\s+(\d+)", body)
        return int(m.group(1)) if m else default
    nfv = num(".amdhsa_next_free_vgpr")
    return {"next_free_vgpr": nfv, "arch_vgprs": num("; num_vgpr"), "agprs": num("; num_agpr", 0),
            "alloc": (nfv + GRANULE - 1) // GRANULE * GRANULE, "lds": num(".amdhsa_group_segment_fixed_size", 0),
            "scratch": num(".amdhsa_private_segment_fixed_size", 0)}


def loop_waits(body):
    """The column loop without guards -- of the blocks that head an innermost loop the one with the most loads (a whole
    ring per iteration; the guarded loop spreads its loads over one block per guard): [(label, global loads, the vmcnt
    values it waits on)]"""
    out = []
    for b in re.split(r"\n(?=\.LBB\d+_\d+:)", body):
        loads = len(re.findall(r"\n\tglobal_load_", b))
        if loads and "Inner Loop Header" in "\n".join(b.split("\n")[:3]):
            out.append((loads, b.split(":")[0], [int(x) for x in re.findall(r"s_waitcnt[^\n]*vmcnt\((\d+)\)", b)]))
    return [(label, loads, waits) for loads, label, waits in sorted(out, reverse=True)[:1]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm-loglik", help="a listing of gh_loglik_mfma.hip made earlier")
    ap.add_argument("--asm-chain", help="a listing of gh_viterbi_chain.hip made earlier")
    ap.add_argument("--keep", metavar="DIR", help="write the listings here")
    a = ap.parse_args()
    d = a.keep or tempfile.mkdtemp(prefix="headline_registers_")
    os.makedirs(d, exist_ok=True)
    todo = [(src, given or os.path.join(d, src[:-4] + ".s"), given is None)
            for (src, _), given in ((LOGLIK, a.asm_loglik), (DECODE, a.asm_chain))]
    with ThreadPoolExecutor(max_workers=2) as ex:
        list(ex.map(lambda t: listing(t[0], t[1]) if t[2] else None, todo))
    res = []
    for (src, tag), (_, path, _) in zip((LOGLIK, DECODE), todo):
        name, body = kernel(open(path).read(), tag)
        m = meta(body)
        res.append((body, m))
        nm = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "")
        print(nm.split("(")[0].replace("void ", ""))
        print("  next_free_vgpr %(next_free_vgpr)d (ArchVGPRs %(arch_vgprs)s, AGPRs %(agprs)d)  allocated %(alloc)d  LDS %(lds)d B static  scratch %(scratch)d B" % m)
    for label, loads, waits in loop_waits(res[1][0]):
        print("  decode column loop without guards (%s): %d global loads per iteration, waits on vmcnt %s" % (label, loads, sorted(set(waits))))
        if not waits or min(waits) == 0:
            print("  WARNING: the loop waits for every load in flight (vmcnt(0)) or not at all")
    ll, dec = res[0][1], res[1][1]
    total = 2 * ll["alloc"] + dec["alloc"]
    ok = total <= SIMD_REGISTERS and not ll["scratch"] and not dec["scratch"]
    print("2 x %d + %d = %d %s %d  ->  %s" % (ll["alloc"], dec["alloc"], total, "<=" if total <= SIMD_REGISTERS else ">", SIMD_REGISTERS,
                                             "a decode wave fits beside two likelihood waves" if ok else "NOT MET"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
