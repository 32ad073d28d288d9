#!/usr/bin/env python3
"""One hash per kernel of the gfx950 code of every csrc/*.hip, to show that a refactor left the machine code alone.
usage: isa_fingerprint.py [--out FILE] [--against FILE] [file.hip ...]
Compiles with build.py's own FLAGS and per-file EXTRA plus --cuda-device-only -S (no GPU is opened), drops the lines that name the
per-compilation __hip_cuid_ symbol, and prints "<file> <symbol> <hash>" for every kernel (and device function that was not
inlined): its instructions, from its label to its kernel descriptor (or function end), with the function's index taken out of
its local labels (.LBB<k>_<n>: a kernel instantiated in front of another renumbers them and changes nothing else);
comments dropped and the kernel's own name blanked; "<file> <symbol>.kd <hash>" for its .amdhsa_kernel block (kernarg size,
register counts ...), and "<file> <rest> <hash>" for what is left (LDS and constant objects, metadata).  --out writes that
listing; --against exits 1 and names what differs, is new, is gone, or has the same code under a new name (a template
parameter more).  A listing is comparable only with listings of this version of the tool: write the parent's with it as well."""
import hashlib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "speech-recognition_amd"))
import build


def fingerprint(src):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "a.s")
        cmd = [build.HIPCC] + build.FLAGS + build.EXTRA.get(src, []) + ["--cuda-device-only", "-S", os.path.join(build.CSRC, src), "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n%s\n%s" % (" ".join(cmd), r.stdout))
        lines = [l for l in open(out).read().split("\n") if "__hip_cuid_" not in l]
    h = lambda ls: hashlib.sha256("\n".join(ls).encode()).hexdigest()[:16]
    res, rest, i = [], [], 0
    while i < len(lines):
        m = re.match(r"([\w.$]+):", lines[i])
        if m and i and lines[i - 1].strip().startswith(".type\t" + m.group(1) + ",@function"):
            j = next(k for k in range(i, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[k]))
            kd = next((k for k in range(i, j) if lines[k].strip().startswith(".amdhsa_kernel ")), j)
            own = lambda l: l.replace(m.group(1)[2:], "@")            # (the kernel's own name, also inside the names of its LDS objects)
            code = [own(re.sub(r"\.L(BB|tmp|func_begin|JTI)\d+_", r".L\1_", l.split(";")[0].rstrip())) for l in lines[i:kd]]
            res.append("%s %s %s" % (src, m.group(1), h(code)))
            if kd < j:
                res.append("%s %s.kd %s" % (src, m.group(1), h([own(l) for l in lines[kd:j]])))
            i = j
        else:
            rest.append(lines[i])
            i += 1
    return res + ["%s <rest> %s" % (src, h(rest))]


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = {}
    for o in ("--out", "--against"):
        if o in args:
            opt[o] = args[args.index(o) + 1]
            del args[args.index(o):args.index(o) + 2]
    srcs = [os.path.basename(a) for a in args] or build._sources()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        listing = [l for r in ex.map(fingerprint, srcs) for l in r]
    text = "\n".join(listing) + "\n"
    if "--out" in opt:
        open(opt["--out"], "w").write(text)
    else:
        sys.stdout.write(text)
    diffs = []
    if "--against" in opt:
        key = lambda l: l.rsplit(" ", 1)[0]
        old = {key(l): l for l in open(opt["--against"]).read().splitlines() if l.split(" ", 1)[0] in srcs}
        new = {key(l): l for l in listing}
        hash_of = lambda l: l.rsplit(" ", 1)[1]
        fresh = {}                                                      # (file, hash) -> a new symbol with that code
        for k in new:
            if k not in old:
                fresh.setdefault((k.split(" ")[0], hash_of(new[k])), k)
        renamed = {k: fresh[(k.split(" ")[0], hash_of(old[k]))] for k in old if k not in new and (k.split(" ")[0], hash_of(old[k])) in fresh}
        diffs = (["differs " + k for k in new if k in old and old[k] != new[k]] +
                 ["new " + k for k in new if k not in old and k not in renamed.values()] +
                 ["renamed, same code: %s -> %s" % (k, v.split(" ")[1]) for k, v in renamed.items()] +
                 ["gone " + k for k in old if k not in new and k not in renamed])
        if diffs:
            print("\n".join(diffs), file=sys.stderr)
    print("%d files, %d kernels, %d differences" % (len(srcs), sum(not l.split(" ")[1].endswith(".kd") for l in listing) - len(srcs),
                                                    len(diffs)), file=sys.stderr)
    sys.exit(1 if diffs else 0)
