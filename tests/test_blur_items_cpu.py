"""k_blur's work items without a GPU: morb_slam_amd/csrc/blur_items.h numbers the 8-px x 24-row strips of an image linearly across its
levels, and the kernel turns an item number back into (level, column, row) with a span search and one 24-bit multiply.  The mapping is
compiled on the host with sanitizers (tests/native/blur_items_check.cc) and walked item by item: every pixel of every level is
covered exactly once, no item starts outside its level, the division is exact, and an image takes ceil(items / 64) waves (94 for
752 x 480).  The built kernel's register budget (five waves per SIMD, no scratch, no LDS) is read from the code object."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "morb_slam_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"


def test_blur_items_cover_every_level_once_under_sanitizers(tmp_path):
    exe = str(tmp_path / "blur_items_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, "-o", exe, os.path.join(NATIVE, "blur_items_check.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert int(re.search(r"cases (\d+)", out.stdout).group(1)) >= 10   # every pyramid of the list really ran


def test_blur_kernel_register_budget():
    """At most 96 VGPRs (five waves per SIMD), no scratch, no LDS: read from the kernel's metadata in the built library."""
    lib = os.path.join(ROOT, "morb_slam_amd", "libmorb_hip.so")
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not (os.path.exists(lib) and all(shutil.which(t) for t in tools)):
        pytest.skip("library or LLVM tools not available")
    import tempfile
    found = []
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([tools[0], "--dump-section", ".hip_fatbin=" + fat, lib])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
        for i, st in enumerate(starts):
            en = starts[i + 1] if i + 1 < len(starts) else len(blob)
            bun, co = os.path.join(tmp, f"bundle{i}.bin"), os.path.join(tmp, f"code{i}.o")
            open(bun, "wb").write(blob[st:en])
            subprocess.check_call([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--input=" + bun, "--output=" + co])
            notes = subprocess.run([tools[2], "--notes", co], capture_output=True, text=True, check=True).stdout
            for kern in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", kern)
                if name and re.search(r"\d+k_blurE", name.group(1)):
                    found.append({k: int(re.search(r"\." + k + r":\s+(\d+)", kern).group(1))
                                  for k in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count")})
    assert len(found) == 1, found
    m = found[0]
    assert m["vgpr_count"] <= 96 and m["private_segment_fixed_size"] == 0 and m["group_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
