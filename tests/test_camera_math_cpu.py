"""include/morb/camera_math.h without a GPU: its host build against the oracle's independent KannalaBrandt8 (oracle/fisheye.cc), bit for
bit, in a program of its own built with the host sanitizers (tests/native/camera_math_check.cc), and the text of the tree: the camera
models and the 4 x 4 null vector are written once."""
import glob
import os
import re
import subprocess

import pytest

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """(exit status, standard output) of the program, built and run once."""
    oracle_lib.build()
    exe = str(tmp_path_factory.mktemp("camera_math") / "camera_math_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(NATIVE, "camera_math_check.cc"),
                           os.path.join(oracle_lib.ORACLE_DIR, "liboracle.so"), "-Wl,-rpath," + oracle_lib.ORACLE_DIR])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    return out.returncode, out.stdout


def test_header_is_the_oracle_bit_for_bit_under_sanitizers(check_output):
    rc, text = check_output
    assert rc == 0 and text.splitlines()[-1] == "mismatches 0" and "FAILED" not in text, text[-2000:]
    counts = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^(\w+) cases (\d+) mismatches (\d+)$", text, re.M)}
    assert set(counts) == {"project", "unproject", "project_d", "project_jac", "triangulate_matches"}
    for name, (cases, mismatches) in counts.items():
        assert mismatches == 0 and cases >= 60000, name
    assert counts["project"][0] >= 300000 and counts["project_d"][0] >= 100000


def test_triangulate_matches_generator_reaches_every_return(check_output):
    """Accepted and each of -1 .. -5 come out of the seeded generator (-3 only through its random rotations; one hand-made case in the
    program reaches it as well)."""
    _, text = check_output
    m = re.search(r"^triangulate_matches histogram accepted (\d+) -1 (\d+) -2 (\d+) -3 (\d+) -4 (\d+) -5 (\d+)$", text, re.M)
    assert m, text[-2000:]
    hist = [int(g) for g in m.groups()]
    assert all(h >= 100 for h in hist), hist


def _sources():
    return sorted(glob.glob(os.path.join(ROOT, "morb_slam_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "include", "**", "*.h"), recursive=True))


def _files_with(pattern):
    return [os.path.relpath(f, ROOT) for f in _sources() if os.path.isfile(f) and re.search(pattern, open(f, errors="replace").read())]


def test_camera_models_and_null_vector_are_written_once():
    assert not os.path.exists(os.path.join(ROOT, "morb_slam_amd", "csrc", "kb8.h"))
    # the KannalaBrandt8 polynomial: the shared header, and sim3.hip's FP64 form with its one sincos
    assert _files_with(r"\btheta9\b") == ["include/morb/camera_math.h", "morb_slam_amd/csrc/sim3.hip"]
    # the 30-sweep Jacobi of the 4 x 4 A^T A (the register Jacobis jrot<P, Q> and jacobi_reg<M> are other algorithms)
    assert _files_with(r"double M\[16\], V\[16\];(?s:.*?)sweep < 30") == ["include/morb/camera_math.h"]
    for name in ("morbkb8", "nmp_project", "nmp_unproject", "nmp_null_vector4", "kb8_project_dev", "kb8_project_f", "q_rotate_f", "Cam9",
                 "MORB_NMP_ATAN2F"):
        assert _files_with(r"\b" + name + r"\b") == [], name
