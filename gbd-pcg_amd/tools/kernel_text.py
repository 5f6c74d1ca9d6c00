#!/usr/bin/env python3
"""One line per kernel symbol of the given .hip files: symbol, line count and hash of its normalised gfx950 text (the instruction
stream and the .amdhsa_ directives), from hipcc -S --offload-device-only with the flags of the Makefile (no GPU needed).
    python gbd-pcg_amd/tools/kernel_text.py gbd-pcg_amd/csrc/pinv*.hip > new.txt      (the same in the other tree, then diff)
Normalised: comments, debug and file directives dropped, local labels renumbered in order of appearance inside the symbol, and
the lines sorted by symbol, so that moving a kernel to another file or to another place in its file changes nothing.  --dump DIR
also writes each symbol's normalised text to DIR/<symbol>.s, to diff one kernel of two trees."""
import hashlib, os, re, subprocess, sys, tempfile
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-result -ffp-contract=off".split()
args = sys.argv[1:]
dump = None
if args and args[0] == "--dump":
    dump, args = args[1], args[2:]
    os.makedirs(dump, exist_ok=True)


def normalise(lines):
    labels, out = {}, []

    def renumber(m):
        return labels.setdefault(m.group(0), f".L{len(labels)}")

    for ln in lines:
        ln = ln.split(";", 1)[0].strip()
        if not ln or re.match(r"\.(file|loc|cfi_|ident|p2align|section|text|type|size|globl|weak|protected|hidden)\b", ln):
            continue
        out.append(re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", renumber, ln))
    return out


rows = {}
for f in args:
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "unit.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-S", "--offload-device-only", f, "-o", asm], check=True)
        text = open(asm).read().splitlines()
    kernels = {m.group(1) for ln in text if (m := re.match(r"\s*\.amdhsa_kernel (\S+)", ln))}
    body, descr, cur = {}, {}, None   # cur: the list the current line belongs to
    for ln in text:
        m = re.match(r"(\S+):", ln)
        if m and m.group(1) in kernels:
            cur = body.setdefault(m.group(1), [])
        elif re.match(r"\.Lfunc_end\d+:", ln) or ".end_amdhsa_kernel" in ln:
            cur = None
        elif (m := re.match(r"\s*\.amdhsa_kernel (\S+)", ln)):
            cur = descr.setdefault(m.group(1), [])
        elif cur is not None:
            cur.append(ln)
    for k in kernels:
        assert body[k] and descr[k] and k not in rows, k
        rows[k] = normalise(body[k]) + normalise(descr[k])
for k in sorted(rows):
    if dump:
        with open(os.path.join(dump, k + ".s"), "w") as fh:
            fh.write("\n".join(rows[k]) + "\n")
    print(k, len(rows[k]), hashlib.sha256("\n".join(rows[k]).encode()).hexdigest()[:16])
