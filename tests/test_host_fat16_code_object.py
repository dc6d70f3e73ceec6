"""Register and scratch budget of every `k_rbf_fat_apply16` instance (csrc/mfx_rbf_fat.hip), read from the code objects of the BUILT
libmfx.so the way tests/test_host_cpu.py reads the scratch budget: llvm-objdump --offloading extracts the gfx950 code objects,
llvm-readelf --notes prints their AMDGPU metadata.

The kernel is written for ONE wave per SIMD: a gfx950 SIMD has 512 registers per lane, of which a wave may own all -- at most 256
architectural VGPRs and 256 accumulation registers (the metadata's .vgpr_count is the unified total, .agpr_count the accumulation
part).  Its tile loop runs two tiles per iteration and has a peeled copy of a tile behind it; none of that may cost scratch: a spill
inside the sweep is a memory access per tile on the kernel that is two thirds of a training step."""

import os
import re
import shutil
import subprocess
import tempfile

import pytest

from matfree_extensions import _lib

OBJDUMP, READELF = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"


def _fat16_metadata():
    """{mangled kernel name: {metadata key: value}} of every k_rbf_fat_apply16 instance"""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF) and os.path.exists(_lib.LIB_PATH)):
        pytest.skip("needs the ROCm llvm tools and a built libmfx.so")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = shutil.copy(_lib.LIB_PATH, os.path.join(tmp, "libmfx.so"))
        subprocess.run([OBJDUMP, "--offloading", so], cwd=tmp, check=True, capture_output=True)  # extracts the bundles next to the copy
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([READELF, "--notes", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            for block in re.split(r"\n\s+- (?=\.agpr_count:)", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", block)
                if not name or "k_rbf_fat_apply16" not in name.group(1):
                    continue
                num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))  # noqa: E731
                out[name.group(1)] = {k: num(k) for k in ("agpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                          "private_segment_fixed_size", "max_flat_workgroup_size")}
    return out


def test_every_fat16_instance_fits_one_wave_per_simd_without_scratch():
    meta = _fat16_metadata()
    # the instances the launch dispatches to: padded dimension 4 and 8, with and without float4 epilogue
    for dpad in (4, 8):
        for vec4 in (0, 1):
            assert any(f"k_rbf_fat_apply16ILi{dpad}ELb{vec4}E" in name for name in meta), (dpad, vec4, sorted(meta))
    assert len(meta) == 4, sorted(meta)
    for name, m in meta.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        # one wave per SIMD: the whole 512-register file of a lane at the most, in its two halves
        assert m["vgpr_count"] <= 512, (name, m)
        assert m["agpr_count"] <= 256 and m["vgpr_count"] - m["agpr_count"] <= 256, (name, m)
        assert m["max_flat_workgroup_size"] == 256, (name, m)  # four waves, one per SIMD of the compute unit
