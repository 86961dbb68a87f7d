"""The host side the two bundle adjusters share, without a GPU: morb_slam_amd/csrc/ba_host.h — the two-pass carve of one device block
into arrays, the CSR lists and 64-edge chunks of the flattened graph, the Schur product's block lists — compiled on the host with
sanitizers (tests/native/ba_host_check.cc) and compared there with the loops LocalBA and LocalInertialBA had before the header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "morb_slam_amd", "csrc")


def test_carver_and_graph_lists_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ba_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, "-o", exe, os.path.join(NATIVE, "ba_host_check.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    # the sweep really ran: 147 request lists, each also with every request grown, dropped and moved to the other region; 2 + 14 + 400
    # graphs; 40 block-list sizes
    carver, graph, blocks = map(int, re.search(r"carver cases (\d+), graph cases (\d+), block-list cases (\d+)", out.stdout).groups())
    assert carver > 147 * 3 and graph == 416 and blocks == 40
    assert int(re.search(r"^cases (\d+)", out.stdout, re.M).group(1)) == carver + graph + blocks


def test_the_adjusters_size_and_carve_through_the_shared_header():
    """One definition of the rounding, of the carve and of the graph lists: neither adjuster keeps a copy, and LocalInertialBA no longer
    lists its sizes apart from the calls that take the memory."""
    hdr = open(os.path.join(CSRC, "ba_host.h")).read()
    assert "hip_runtime" not in hdr and "#include <hip" not in hdr and "#include \"" not in hdr   # g++ compiles it alone
    for name in ("class ArenaCarver", "void csr_by_key(", "void chunks_of(", "void schur_block_lists("):
        assert name in hdr, name
    for name in ("inertial_ba.hip", "local_ba.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert '#include "ba_host.h"' in src, name
        assert "& ~(size_t)255" not in src and "blkIndex[(size_t)bi *" not in src, name
        assert "ArenaCarver" in src and "csr_by_key(" in src and "chunks_of(" in src and "schur_block_lists(" in src, name
    for name in ("inertial.hip", "inertial_ba.hip"):   # (LocalInertialBA lived in inertial.hip before it had a unit of its own)
        inertial = open(os.path.join(CSRC, name)).read()
        assert "& ~(size_t)255" not in inertial and "blkIndex[(size_t)bi *" not in inertial, name
        assert "carve-up overflow" not in inertial and not re.search(r"\breserve\b", inertial), name
        for gone in ("dalloc", "upHi", "stageCap", "cleanup", "arenaBytes"):
            assert not re.search(r"\b%s\b" % gone, inertial), (name, gone)
