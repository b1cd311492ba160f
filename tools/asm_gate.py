#!/usr/bin/env python3
"""The refactor gate: did a change leave every kernel's machine code alone?

    make -C lz4_frame_conduit_amd/csrc asm          # in a checkout of the parent, and in this tree
    tools/asm_gate.py PARENT.s THIS.s [--renamed OLD=NEW ...]

PARENT.s and THIS.s are the engine-hip-amdgcn-amd-amdhsa-gfx950.s files that `make asm` leaves in lz4_frame_conduit_amd/build/asm.
Both are split per kernel.  Of a kernel's body the labels and the instructions stay, directives and comments go; label numbers and
mangled symbols are masked, since both move when a kernel is added, removed or renamed anywhere in the file.  For every kernel of
the parent one line: EQUAL, or DIFF with the first line that differs, then both instruction counts and the resource figures (the
.amdhsa_* directives and the kernel-info comment: VGPRs, SGPRs, LDS, scratch, occupancy).  A kernel is EQUAL when the whole masked
stream and the figures are; nothing is searched for inside a stream.  Kernels that only THIS.s has are listed as new.

--renamed OLD=NEW pairs a kernel of the parent with its new name.  Either side is a mangled name, or the demangled name without
return type and argument list as this tool prints it, e.g. 'lz4f::k_bc_find_solo_set=lz4f::k_bc_find_solo<true, true, lz4f::DsView>'.

Exit status 1: a kernel of the parent differs, or is missing without a --renamed entry.
"""
import argparse
import re
import shutil
import subprocess
import sys

FIGURES = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"), ("lds", ".amdhsa_group_segment_fixed_size"),
           ("scratch", ".amdhsa_private_segment_fixed_size"), ("kernarg", ".amdhsa_kernarg_size"))
INFO = (("NumVgprs", "NumVgprs"), ("NumAgprs", "NumAgprs"), ("TotalNumSgprs", "TotalNumSgprs"), ("ScratchSize", "ScratchSize"),
        ("LDSByteSize", "LDSByteSize"), ("Occupancy", "Occupancy"))
LABEL = re.compile(r"\.L([A-Za-z_]+)\d+(_\d+)?")        # .LBB46_12 -> .LBB_12: the first number is the function's place in the file
SYMBOL = re.compile(r"\b_Z\w+")


def mask(line):
    line = line.split(";", 1)[0].strip()
    line = LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)
    return SYMBOL.sub("SYM", line)


def kernels_of(path):
    """{mangled name: {"code": [masked lines], "n": instruction count, "fig": {name: value}}}, in the file's order"""
    with open(path) as f:
        lines = f.read().split("\n")
    names = [ln.split()[1] for ln in lines if ln.lstrip().startswith(".amdhsa_kernel ")]
    wanted = set(names)
    out, cur, in_body, in_desc, in_info = {}, None, False, False, False
    for ln in lines:
        s = ln.strip()
        if not in_body and ":" in s and not ln[:1].isspace() and s.split(":", 1)[0] in wanted:      # NAME:  ; @NAME
            cur = out[s.split(":", 1)[0]] = {"code": [], "n": 0, "fig": {}}
            in_body, in_info = True, False
            continue
        if cur is None:
            continue
        if in_body:
            if s.startswith(".amdhsa_kernel "):
                in_desc = True
            elif s == ".end_amdhsa_kernel":
                in_desc = False
            elif in_desc:
                for key, directive in FIGURES:
                    if s.startswith(directive + " "):
                        cur["fig"][key] = s.split()[1]
            elif s.startswith(".Lfunc_end"):
                in_body = False
            elif s and not s.startswith(";"):
                m = mask(s)
                if m.endswith(":"):
                    cur["code"].append(m)
                elif m and not m.startswith("."):
                    cur["code"].append(m)
                    cur["n"] += 1
        elif s == "; Kernel info:":
            in_info = True
        elif in_info and s.startswith(";"):
            for key, word in INFO:
                m = re.match(r";\s*%s:\s*(\d+)" % word, s)
                if m:
                    cur["fig"][key] = m.group(1)
        elif in_info:
            in_info, cur = False, None
    missing = [n for n in names if n not in out]
    if missing:
        sys.exit("%s: no body found for %s" % (path, ", ".join(missing)))
    return out


def demangler():
    for tool in ("llvm-cxxfilt", "c++filt"):
        exe = shutil.which(tool)
        if exe:
            return exe
    return None


def short_names(names):
    """mangled -> demangled, without the return type and the argument list (mangled itself where no demangler is installed)"""
    exe = demangler()
    if not exe or not names:
        return {n: n for n in names}
    full = subprocess.run([exe], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for n, d in zip(names, full):
        if d.startswith("void "):
            d = d[5:]
        depth = 0
        for i, c in enumerate(d):
            depth += (c == "<") - (c == ">")
            if c == "(" and depth == 0:
                d = d[:i]
                break
        out[n] = d
    return out


def figures(k):
    return " ".join("%s=%s" % (key, k["fig"].get(key, "?")) for key, _ in FIGURES + INFO)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--quiet", action="store_true", help="print only DIFF, MISSING, renamed and new kernels, and the summary")
    args = ap.parse_args()
    old, new = kernels_of(args.parent), kernels_of(args.this)
    old_short, new_short = short_names(list(old)), short_names(list(new))

    def find(word, table, shorts):
        hits = [n for n in table if word in (n, shorts[n])]
        if len(hits) != 1:
            sys.exit("--renamed: %r names %d kernels" % (word, len(hits)))
        return hits[0]

    renamed = {}
    for pair in args.renamed:
        a, _, b = pair.partition("=")
        renamed[find(a, old, old_short)] = find(b, new, new_short)
    bad, paired = 0, set()
    for name, k in old.items():
        to = renamed.get(name, name)
        label = old_short[name] + (" -> " + new_short[to] if to != name else "")
        if to not in new:
            print("MISSING  %s" % label)
            bad += 1
            continue
        paired.add(to)
        t = new[to]
        diff = next((i for i, (a, b) in enumerate(zip(k["code"], t["code"])) if a != b), None)
        if diff is None and len(k["code"]) != len(t["code"]):
            diff = min(len(k["code"]), len(t["code"]))
        if diff is None and k["fig"] == t["fig"]:
            if not args.quiet or to != name:
                print("EQUAL    %s  %d instructions  %s" % (label, k["n"], figures(k)))
            continue
        bad += 1
        print("DIFF     %s  %d -> %d instructions" % (label, k["n"], t["n"]))
        if diff is not None:
            print("    first at line %d:  %s  |  %s" % (diff, (k["code"] + ["<end>"])[diff], (t["code"] + ["<end>"])[diff]))
        print("    parent: %s\n    this:   %s" % (figures(k), figures(t)))
    for name, k in new.items():
        if name not in paired:
            print("NEW      %s  %d instructions  %s" % (new_short[name], k["n"], figures(k)))
    print("%d kernels of the parent: %d equal, %d differ or are missing; %d new" % (len(old), len(old) - bad, bad, len(new) - len(paired)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
