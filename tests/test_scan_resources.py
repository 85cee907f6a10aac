"""The two-pass list scan's register and LDS budget, read from the built code object.

k_scan_lean<16, JB, true> is resident three workgroups per CU only while it
stays within 168 VGPRs (512 / 3 waves per SIMD, in steps of 8) and about 53 KB of
LDS (160 KB / 3), and it must not use scratch: the compiler obeys
__launch_bounds__(256, 3) by spilling, silently.  The kernel reaches the budget
only through hand-placed rematerialisation (opq() in ivfpq_kernels.hip), so an
unrelated edit of its item loop or a compiler update can undo it.  This test
reads the metadata the compiler wrote for the gfx950 code object of the build.
"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OBJ = os.path.join(HERE, "..", "chameleon-rag-acceleration_amd", "lib", "ivfpq_kernels.o")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")

MAX_VGPRS = 168
MAX_LDS = 53 * 1024


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    assert os.path.exists(OBJ), f"{OBJ} missing: run __graft_entry__.build() first"
    tmp = tmp_path_factory.mktemp("co")
    fat, co = str(tmp / "fat.bin"), str(tmp / "kernels.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", OBJ, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    # one metadata record per kernel, each opening with "  - .agpr_count:"
    for rec in re.split(r"\n  - \.", notes):
        name = re.search(r"^    \.name:\s+(\S+)\s*$", rec, re.M)
        if not name:
            continue
        f = {}
        for key in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            f[key] = int(re.search(rf"^    \.{key}:\s+(\d+)\s*$", rec, re.M).group(1))
        out[name.group(1)] = f
    return out


def test_two_pass_scan_fits_three_workgroups_per_cu(kernels):
    split = {n: f for n, f in kernels.items() if re.search(r"k_scan_leanILi16ELi\d+ELb1E", n)}
    assert len(split) == 1, f"expected one k_scan_lean<16, JB, true>, found {sorted(split)}"
    (name, f), = split.items()
    print(name, f)
    assert f["private_segment_fixed_size"] == 0, f"scratch: {f}"
    assert f["vgpr_spill_count"] == 0, f
    assert f["vgpr_count"] <= MAX_VGPRS, f
    assert f["group_segment_fixed_size"] <= MAX_LDS, f


def test_one_pass_scans_use_no_scratch(kernels):
    lean = {n: f for n, f in kernels.items() if "k_scan_leanILi" in n}
    assert len(lean) >= 2, sorted(lean)
    for n, f in lean.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (n, f)
