#!/usr/bin/env python3
"""Are the gfx950 kernels of two source trees textually the same assembly?  (no GPU needed)

  hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S csrc/FILE.hip -o FILE.s        # for every file on either side
  python tools/asm_identity.py --old OLD/mfx_rbf_mfma.s --new NEW/mfx_rbf_mfma.s NEW/mfx_rbf_mfma_grad.s

Every kernel is cut out of the compiler's assembly from its function label through `.end_amdhsa_kernel`: the instruction stream
and every .amdhsa_* directive (registers, LDS, scratch, workgroup size).  Two things that say WHERE a kernel stands and nothing
about WHAT it is are replaced by placeholders: the kernel's own mangled name, and its ordinal within the file in the compiler's
local labels (.LBB<ordinal>_<block>, .Lfunc_end<ordinal>).  The kernels are then paired by name and compared as plain text.
The one renaming known here: k_rbf_mfma_apply_h3<DPAD, NB, VEC4, KIND, DH, PK> of the old tree pairs with k_rbf_h3_packed<DPAD, NB,
VEC4, KIND> (DH = PK = 1) and k_rbf_h3_split<...> (DH = PK = 0).  Prints one line per kernel, then the totals; exit status 1 if a
pair differs or a kernel has no partner."""
import argparse
import re
import sys

H3_OLD = re.compile(r"^_ZN3mfx19k_rbf_mfma_apply_h3ILi(\d+)ELi(\d+)ELb([01])ELi(\d+)ELb([01])ELb([01])EEEv")
H3_NEW = re.compile(r"^_ZN3mfx\d+k_rbf_h3_(packed|split)ILi(\d+)ELi(\d+)ELb([01])ELi(\d+)EEEv")


def key_of(sym):
    m = H3_OLD.match(sym)
    if m:
        dpad, nb, vec4, kind, dh, pk = m.groups()
        which = {"11": "packed", "00": "split"}.get(dh + pk, f"DH{dh}PK{pk}")
        return f"h3_{which}<DPAD {dpad}, NB {nb}, VEC4 {vec4}, KIND {kind}>"
    m = H3_NEW.match(sym)
    if m:
        which, dpad, nb, vec4, kind = m.groups()
        return f"h3_{which}<DPAD {dpad}, NB {nb}, VEC4 {vec4}, KIND {kind}>"
    return sym


def kernels(paths):
    """{pairing key: normalised text of the kernel}"""
    out = {}
    for path in paths:
        lines = open(path).read().split("\n")
        start = {}
        for i, line in enumerate(lines):
            m = re.match(r"^(\w+):\s", line + " ")
            if m:
                start[m.group(1)] = i
            m = re.match(r"^\s*\.amdhsa_kernel (\S+)", line)
            if m:
                sym = m.group(1)
                end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
                text = "\n".join(lines[start[sym]:end + 1]).replace(sym, "SELF")
                # .LBB<ordinal>_<block>, and BB<ordinal>_<block> in the loop comments -- as whole tokens only
                text = re.sub(r"(?<![\w.$])(\.L)?BB\d+_(\d+)(?![\w.$])", r"\1BBN_\2", text)
                text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1N", text)
                text = re.sub(r"[ \t]+;", " ;", text)  # the comment column moves with the width of a label
                assert key_of(sym) not in out, sym
                out[key_of(sym)] = text
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    same = differ = 0
    for k in sorted(set(old) | set(new)):
        if k not in new:
            print("only in old  ", k)
        elif k not in old:
            print("only in new  ", k)
        elif old[k] == new[k]:
            same += 1
            print("identical    ", k)
        else:
            differ += 1
            print("DIFFERS      ", k, f"({old[k].count(chr(10)) + 1} -> {new[k].count(chr(10)) + 1} lines)")
    unmatched = len(set(old) ^ set(new))
    count = lambda d, w: sum(k.startswith(f"h3_{w}<") for k in d)  # noqa: E731
    print(f"kernels: old {len(old)}, new {len(new)}; h3 packed {count(old, 'packed')} / {count(new, 'packed')}, "
          f"h3 split {count(old, 'split')} / {count(new, 'split')}")
    print(f"identical {same}, differing {differ}, unmatched {unmatched}")
    return 1 if differ or unmatched else 0


if __name__ == "__main__":
    sys.exit(main())
