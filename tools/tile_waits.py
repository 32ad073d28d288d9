#!/usr/bin/env python3
"""Where the operand-ring loads and their waits sit among the MFMAs of the matrix-core likelihood kernel's tile loop.

The A fragments of loglik_mfma_kernel travel through a register ring: a slot is meant to be refilled right
behind the MFMA pair that consumed it and waited for only where it is consumed next, so that every load has a ring's
length of MFMAs to return from L2.  Whether the compiled kernel does that is a property of the listing, not of the
source: the scheduler is free to batch the loads and the wait-count pass then has to drain them.  This tool compiles
csrc/gh_loglik_mfma.hip for gfx950 exactly as build.py does (device side only, to assembly; ~3 min; no GPU), finds the
tile blocks of the named instantiations as tools/epilogue_isa.py does, and prints for each block

  * the order of MFMAs, global loads and `s_waitcnt vmcnt(N)`:  M = one MFMA, L = one global load, wN = a wait for all
    but the youngest N loads, .k = k other vector instructions (the epilogue of the tile before);
  * the smallest vmcnt in front of the first MFMA pair (0 = every load in flight has to land before the tile starts);
  * for every global load the distance, in MFMAs, to the first MFMA that reads its destination (following the loop
    into the next tile block): the real run-ahead of the ring.  Loads not read by an MFMA of the loop are left out.

    python tools/tile_waits.py                       # every fp64 instantiation with 20 k-steps (D <= 40)
    python tools/tile_waits.py double,20,8,false,false,true float,20,8,false     # T,KS,MP,MULTI,FE,BND
    python tools/tile_waits.py --asm listing.s ...   # a listing made earlier (--keep writes one)
"""
import argparse
import importlib.util
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def _epilogue_isa():
    spec = importlib.util.spec_from_file_location("epilogue_isa", os.path.join(HERE, "epilogue_isa.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def regs(operand):
    """v[10:11] -> {10, 11}, v7 -> {7}; anything else -> empty"""
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", operand)
    return {int(m.group(1))} if m else set()


def operands(ins):
    parts = ins.split(None, 1)
    return [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []


def events(ins_list):
    """[(kind, payload)]: ("M", source registers), ("L", destination registers), ("w", N), (".", None) for other vector ops"""
    out = []
    for ins in ins_list:
        op = ins.split()[0]
        if op.startswith("v_mfma"):
            ops = operands(ins)
            out.append(("M", set().union(*[regs(o) for o in ops[1:]])))
        elif op.startswith("global_load"):
            out.append(("L", regs(operands(ins)[0])))
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", ins)
            if m:
                out.append(("w", int(m.group(1))))
        elif op.startswith("v_"):
            out.append((".", None))
    return out


def sequence(ev):
    toks, dots = [], 0
    for kind, val in ev:
        if kind == ".":
            dots += 1
            continue
        if dots:
            toks.append(".%d" % dots)
            dots = 0
        toks.append("w%d" % val if kind == "w" else kind)
    if dots:
        toks.append(".%d" % dots)
    # runs of one token: M M M M -> Mx4
    out = []
    for t in toks:
        if out and out[-1][0] == t and t in ("M", "L"):
            out[-1][1] += 1
        else:
            out.append([t, 1])
    return " ".join(t if n == 1 else "%sx%d" % (t, n) for t, n in out)


def distances(blocks_ev, k):
    """For every load of block k: (MFMAs of the block issued before it, MFMAs between it and the first MFMA that reads its
    destination), following the loop into the next tile block"""
    res = []
    ev = blocks_ev[k]
    follow = ev + blocks_ev[(k + 1) % len(blocks_ev)] + ev
    n_before = 0
    for i, (kind, val) in enumerate(ev):
        if kind == "M":
            n_before += 1
        if kind != "L" or not val:
            continue
        d = 0
        for kind2, val2 in follow[i + 1:]:
            if kind2 == "L" and val2 & val:
                break                       # overwritten before any MFMA read it: not an operand of this loop
            if kind2 == "M":
                if val2 & val:
                    res.append((n_before, d))
                    break
                d += 1
    return res


def report(E, name, body):
    blocks, n_mfma = E.tile_blocks(body)
    reg = {k: re.search(re.escape(k) + r"\s+(\S+)", body).group(1) for k in (".amdhsa_next_free_vgpr", ".amdhsa_accum_offset")
           if re.search(re.escape(k) + r"\s+(\S+)", body)}
    print("%s  %s" % (name, reg))
    blocks_ev = [events(b) for b in blocks]
    for k, ev in enumerate(blocks_ev):
        loads = sum(kind == "L" for kind, _ in ev)
        first_m = next(i for i, (kind, _) in enumerate(ev) if kind == "M")
        head = [v for kind, v in ev[:first_m] if kind == "w"]
        waits = [v for kind, v in ev if kind == "w"]
        dist = distances(blocks_ev, k)
        print("  tile block %d of %d: %d MFMAs, %d global loads, %d vmcnt waits" % (k + 1, len(blocks_ev), n_mfma, loads, len(waits)))
        print("    order: " + sequence(ev))
        print("    smallest vmcnt in front of the first MFMA pair: %s;  all waits in order: %s"
              % (min(head) if head else "none", " ".join(map(str, waits)) or "none"))
        if dist:
            print("    refill -> use, in MFMAs (issued behind MFMA #: distance): " + " ".join("%d:%d" % d for d in dist))
            print("    run-ahead min %d, max %d, mean %.1f MFMAs over %d loads" % (min(d for _, d in dist), max(d for _, d in dist),
                                                                                 sum(d for _, d in dist) / len(dist), len(dist)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("inst", nargs="*", help="template arguments T,KS,MP,MULTI[,FE[,BND]]; default: every fp64 instantiation with KS = 20")
    ap.add_argument("--asm", help="read this listing instead of compiling")
    ap.add_argument("--keep", help="write the listing here")
    a = ap.parse_args()
    E = _epilogue_isa()
    if a.asm:
        asm = open(a.asm).read()
    else:
        path = a.keep or os.path.join(tempfile.mkdtemp(prefix="tile_waits_"), "gh_loglik_mfma.s")
        E.listing(path)
        asm = open(path).read()
    found = dict(E.kernels(asm))
    if a.inst:
        want = [E.mangled(i) for i in a.inst]
        names = [n for w in want for n in found if w in n]
        if len(names) < len(want):
            sys.exit("not in the listing: %s" % [w for w in want if not any(w in n for n in found)])
    else:
        names = sorted(n for n in found if "loglik_mfma_kernelIdLi20E" in n)
    for n in names:
        report(E, n, found[n])


if __name__ == "__main__":
    main()
