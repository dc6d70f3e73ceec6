#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libmfx.so function by function (no GPU needed).

  python tools/diff_code_objects.py OLD/libmfx.so NEW/libmfx.so

Instructions are compared as llvm-objdump prints them, without addresses, encodings and the padding between functions.  The dense cross sweeps of the old
naming (k_rbf_cross_grad_dense[_wide]<.., TRANS>) are matched with the weight-source instantiations that replaced them
(k_rbf_cross_grad[_wide]<.., DenseSrc<T, TRANS>> / <.., FactoredSrc<T>>), and the two overloads each of k_rbf_mfma_grad[_h] (runtime
families <..>, Matern-5/2 <.., 3>) with the one template that replaced them (<.., false> / <.., true>).  For every function that differs, the register, LDS,
scratch and spill figures of both builds are printed, with the waves per SIMD that the registers allow, and at the end how many of
them gained scratch or spills, changed their LDS size or lost a wave per SIMD.  Exit status 1 if anything differs or is unmatched."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count")


def waves_per_simd(vgprs):
    """gfx950: 512 registers per lane of a SIMD (vector and accumulation registers together), handed out in blocks of 8, at most 8 waves"""
    return min(8, 512 // ((max(vgprs, 1) + 7) // 8 * 8))


def canonical(name):
    """demangled name without the parameter list, cross sweeps in the weight-source naming"""
    name = re.sub(r"^void ", "", name)
    while "> >" in name:
        name = name.replace("> >", ">>")
    name = name[: name.index(">(") + 1] if ">(" in name else name.split("(")[0]
    name = re.sub(r"\.kd$", "", name)
    m = re.match(r"mfx::k_rbf_cross_grad(_dense)?(_wide)?<(float|double), (.*)>$", name)
    if m and "Src<" not in name:
        dense, wide, t, rest = m.groups()
        args = rest.split(", ")
        src = f"mfx::DenseSrc<{t}, {args.pop()}>" if dense else f"mfx::FactoredSrc<{t}>"
        name = f"mfx::k_rbf_cross_grad{wide or ''}<{t}, {', '.join(args)}, {src}>"
    if name.startswith("_ZN3mfx17k_rbf_mfma_grad_hI"):  # (c++filt does not know the _Float16 parameters: stays mangled)
        name = re.sub(r"^(\w+?ILi\d+ELi\d+ELb[01]E)(EEv)", r"\1Lb0E\2", name).replace("ELb0ELi3EEEv", "ELb0ELb1EEEv")
    m = re.match(r"mfx::k_rbf_mfma_grad(_h)?<(.*)>$", name)
    if m and len(m.group(2).split(", ")) == (3 if m.group(1) else 2):  # the runtime-family overload of the old naming
        name = f"mfx::k_rbf_mfma_grad{m.group(1) or ''}<{m.group(2)}, false>"
    elif m and m.group(2).endswith(", 3"):  # ... and its Matern-5/2 overload (KIND = MFX_KERNEL_MATERN52)
        name = f"mfx::k_rbf_mfma_grad{m.group(1) or ''}<{m.group(2)[:-3]}, true>"
    return name


def load(so):
    """{canonical name: (instruction text, {metadata key: value})}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = shutil.copy(so, os.path.join(tmp, "libmfx.so" if so.endswith(".so") else "device-gfx950.co"))
        if so.endswith(".so"):  # (anything else: a device-only code object, `hipcc --cuda-device-only -c`)
            subprocess.run([LLVM + "llvm-objdump", "--offloading", copy], cwd=tmp, check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            path = os.path.join(tmp, f)
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", path], check=True, capture_output=True, text=True).stdout
            meta = {}
            for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
                block = ".agpr_count:" + block
                sym = re.search(r"\.name:\s+(\S+)", block)
                if sym:
                    meta[sym.group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", block).group(1)) for k in KEYS}
            dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", path], check=True, capture_output=True, text=True).stdout
            syms = re.findall(r"^[0-9a-f]+ <(\S+)>:$", dis, flags=re.M)
            names = subprocess.run(["c++filt"], input="\n".join(syms), check=True, capture_output=True, text=True).stdout.split("\n")
            pretty = dict(zip(syms, names))
            for sym, body in re.findall(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <\S+>:$|\Z)", dis, flags=re.M | re.S):
                text = "\n".join(re.sub(r"\s*//.*$", "", line).strip() for line in body.split("\n")
                                 if line.strip() and line.strip() != "...")  # ("...": zero padding behind a function)
                text = text.replace(sym, "SELF")  # branch targets are printed as <symbol+offset>
                out[canonical(pretty[sym])] = (text, meta.get(sym, {}))
    return out


def main():
    old, new = load(sys.argv[1]), load(sys.argv[2])
    same = [n for n in old if n in new and old[n][0] == new[n][0]]
    differ = [n for n in old if n in new and old[n][0] != new[n][0]]
    cross = lambda names: sum("k_rbf_cross_grad" in n and "gx_final" not in n for n in names)  # noqa: E731
    print(f"functions: old {len(old)}, new {len(new)}; identical {len(same)} (cross family {cross(same)}), "
          f"differing {len(differ)} (cross family {cross(differ)})")
    for n in sorted(set(old) - set(new)):
        print("only in old:", n)
    for n in sorted(set(new) - set(old)):
        print("only in new:", n)
    worse = {"scratch or spills gained": 0, "LDS bytes changed": 0, "fewer waves per SIMD": 0}
    for n in sorted(differ):
        print("differs:", n)
        a, b = old[n][1], new[n][1]
        for k in KEYS:
            print(f"    {k}: {a.get(k)} -> {b.get(k)}")
        print(f"    instructions: {old[n][0].count(chr(10)) + 1} -> {new[n][0].count(chr(10)) + 1}")
        if a and b:
            print(f"    waves per SIMD: {waves_per_simd(a['vgpr_count'])} -> {waves_per_simd(b['vgpr_count'])}")
            worse["scratch or spills gained"] += (b["private_segment_fixed_size"] > a["private_segment_fixed_size"]
                                                  or b["vgpr_spill_count"] > a["vgpr_spill_count"])
            worse["LDS bytes changed"] += b["group_segment_fixed_size"] != a["group_segment_fixed_size"]
            worse["fewer waves per SIMD"] += waves_per_simd(b["vgpr_count"]) < waves_per_simd(a["vgpr_count"])
    if differ:
        print("of the differing functions: " + ", ".join(f"{k} {v}" for k, v in worse.items()))
    return 1 if differ or set(old) ^ set(new) else 0


if __name__ == "__main__":
    sys.exit(main())
