"""The split list scan's register and LDS budget, read from the built code object.

The shipped k_scan_lean<16, JB, true, 2>, the two-pass form, ships at THREE
workgroups per CU.  So the budget checked here is the three-per-CU one: at most
168 VGPRs (512 / 3 waves per SIMD, in steps of 8) and 53 KB of static LDS (three
allocations, rounded up to the LDS granule, within 160 KB), and no scratch: the
compiler obeys the launch bounds by spilling, silently.  A four-pass build
(-DSCAN_LEAN_PASSES=4) is compiled for four workgroups per CU and runs four per
CU one batch at a time (with batches in flight its launch caps it at three), so
it must stay within 128 VGPRs and 40 KB.  The kernel is inside these budgets only because the
uniform item fields are returned to SGPRs and per-thread addresses are formed at
their use (readfirstlane and opq() in ivfpq_kernels.hip), so an unrelated edit of
its item loop or a compiler update can undo it.  This test reads the metadata the
compiler wrote for the gfx950 code object of the build.
"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OBJ = os.path.join(HERE, "..", "chameleon-rag-acceleration_amd", "lib", "ivfpq_kernels.o")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")

MAX_VGPRS = {2: 168, 4: 128}                       # three / four waves per SIMD
MAX_LDS = {2: 53 * 1024, 4: 40 * 1024}              # three / four workgroups per CU


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    assert os.path.exists(OBJ), f"{OBJ} missing: run __graft_entry__.build() first"
    tmp = tmp_path_factory.mktemp("co4")
    fat, co = str(tmp / "fat.bin"), str(tmp / "kernels.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", OBJ, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for rec in re.split(r"\n  - \.", notes):  # one metadata record per kernel
        name = re.search(r"^    \.name:\s+(\S+)\s*$", rec, re.M)
        if not name:
            continue
        f = {}
        for key in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
            f[key] = int(re.search(rf"^    \.{key}:\s+(\d+)\s*$", rec, re.M).group(1))
        out[name.group(1)] = f
    return out


def test_shipped_m16_scan_within_its_residency_budget(kernels):
    m16 = {n: f for n, f in kernels.items() if re.search(r"k_scan_leanILi16ELi\d+ELb[01]E", n)}
    assert len(m16) == 1, f"expected one k_scan_lean<16, ...>, found {sorted(m16)}"
    (name, f), = m16.items()
    print(name, f)
    np_ = re.search(r"k_scan_leanILi16ELi\d+ELb1ELi(\d+)EE", name)
    assert np_ and int(np_.group(1)) in MAX_VGPRS, f"not a split form: {name}"
    passes = int(np_.group(1))
    assert f["private_segment_fixed_size"] == 0, f"scratch: {f}"
    assert f["vgpr_spill_count"] == 0, f
    assert f["vgpr_count"] <= MAX_VGPRS[passes], f
    assert f["group_segment_fixed_size"] <= MAX_LDS[passes], f


def test_one_pass_m8_scan_uses_no_scratch(kernels):
    m8 = {n: f for n, f in kernels.items() if re.search(r"k_scan_leanILi8ELi\d+ELb0ELi1EE", n)}
    assert len(m8) == 1, f"expected one one-pass k_scan_lean<8, ...>, found {sorted(m8)}"
    (name, f), = m8.items()
    print(name, f)
    assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, f
