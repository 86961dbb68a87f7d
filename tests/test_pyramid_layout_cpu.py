"""The stored layout of the image pyramid without a GPU: morb_slam_amd/csrc/pyramid_layout.h — three stored border pixels instead of
the reference's nineteen — compiled on the host with sanitizers (tests/native/pyramid_layout_check.cc).  Every reader of the pyramid
(resize, gather, blur, FAST, describe, stereo SAD) must stay inside the buffer and its zeroed tail at every size, scale factor,
level count and image count the program sweeps, rows must be 64-byte aligned with the interior at byte 3, and the bench shape
must take 1 199 552 bytes per image."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "morb_slam_amd", "csrc")


def test_pyramid_layout_extents_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pyramid_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, "-o", exe, os.path.join(NATIVE, "pyramid_layout_check.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert int(re.search(r"cases (\d+)", out.stdout).group(1)) > 300   # the sweep really ran


def test_the_kernels_take_the_stored_pad_from_the_shared_header():
    """One definition of the stored border: the extractor and the matcher address d_pyr with kPyrPad from pyramid_layout.h, and
    neither keeps a pad constant of its own."""
    hdr = open(os.path.join(CSRC, "pyramid_layout.h")).read()
    assert re.search(r"constexpr int kPyrPad = 3;", hdr) and re.search(r"constexpr int EDGE = 19;", hdr)
    for name in ("extractor.hip", "matcher.hip", "extractor_internal.h", "fast_wave.h"):
        src = open(os.path.join(CSRC, name)).read()
        assert not re.search(r"constexpr int (EDGE_?|kPyrPad) *=", src), name
    assert "kPyrPad" in open(os.path.join(CSRC, "matcher.hip")).read()
