"""The host side the bundle adjusters share, without a GPU: morb_slam_amd/csrc/ba_host.h — the two-pass carve of one device block
into arrays, the CSR lists and 64-edge chunks of the flattened graph, the Schur product's block lists, the queue of LM trial slots —
compiled on the host with sanitizers (tests/native/ba_host_check.cc) and compared there with the loops LocalBA and LocalInertialBA had
before the header; the queue runs against a thread that plays the device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "morb_slam_amd", "csrc")


def test_carver_and_graph_lists_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ba_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", "-I" + CSRC, "-o", exe, os.path.join(NATIVE, "ba_host_check.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    # the sweep really ran: 147 request lists, each also with every request grown, dropped and moved to the other region; 2 + 14 + 400
    # graphs; 40 block-list sizes; the slot queue's 3 x 7 runs to `done` (or the limit) and its 6 other cases
    carver, graph, blocks, queue = map(int, re.search(r"carver cases (\d+), graph cases (\d+), block-list cases (\d+), queue cases (\d+)",
                                                       out.stdout).groups())
    assert carver > 147 * 3 and graph == 416 and blocks == 40 and queue == 27
    assert int(re.search(r"^cases (\d+)", out.stdout, re.M).group(1)) == carver + graph + blocks + queue


def test_slot_queue_under_thread_sanitizer(tmp_path):
    """The same program built with ThreadSanitizer, the slot queue's cases alone: the host's acquire loads against the release stores of
    the thread that plays the device."""
    probe = tmp_path / "probe.cc"
    probe.write_text("#include <thread>\nint main() { int x = 0; std::thread t([&] { x = 1; }); t.join(); return x - 1; }\n")
    tsan = ["g++", "-std=c++17", "-O1", "-g1", "-Wall", "-fsanitize=thread", "-pthread"]
    if subprocess.run(tsan + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain does not link, or this kernel does not run, a -fsanitize=thread program")
    exe = str(tmp_path / "ba_host_check_tsan")
    subprocess.check_call(tsan + ["-I" + CSRC, "-o", exe, os.path.join(NATIVE, "ba_host_check.cc")])
    out = subprocess.run([exe, "queue"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    assert "ThreadSanitizer" not in out.stderr and "queue cases 27" in out.stdout and "carver cases 0" in out.stdout


def test_the_adjusters_size_and_carve_through_the_shared_header():
    """One definition of the rounding, of the carve, of the graph lists and of the host loop that queues LM trials: neither unit keeps
    a copy, and LocalInertialBA no longer lists its sizes apart from the calls that take the memory."""
    hdr = open(os.path.join(CSRC, "ba_host.h")).read()
    assert "hip_runtime" not in hdr and "#include <hip" not in hdr and "#include \"" not in hdr   # g++ compiles it alone
    for name in ("class ArenaCarver", "void csr_by_key(", "void chunks_of(", "void schur_block_lists(", "int lm_slot_queue("):
        assert name in hdr, name
    for name in ("inertial_ba.hip", "local_ba.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert '#include "ba_host.h"' in src, name
        assert "& ~(size_t)255" not in src and "blkIndex[(size_t)bi *" not in src, name
        assert "ArenaCarver" in src and "csr_by_key(" in src and "chunks_of(" in src and "schur_block_lists(" in src, name
        # the wait for the LM decisions is the header's: no unit backs off or polls the stream in a loop of its own (the look() it
        # hands to the queue is handles.h's stream_look, which holds the one hipStreamQuery)
        assert "lm_slot_queue(" in src, name
        for gone in ("__builtin_ia32_pause", "sched_yield", "nanosleep", "spins"):
            assert gone not in src, (name, gone)
        assert "hipStreamQuery" not in src and src.count("stream_look(") == 1 and re.search(r"\[&\]\(\) \{ return stream_look\(st, [\w.]+\); \}", src), name
    handles = open(os.path.join(CSRC, "handles.h")).read()
    assert handles.count("hipStreamQuery") == 1 and re.search(r"StreamLook stream_look\(hipStream_t st, const char\* who\) \{\s*const hipError_t e = hipStreamQuery\(st\);", handles)
    for name in ("inertial.hip", "inertial_ba.hip"):   # (LocalInertialBA lived in inertial.hip before it had a unit of its own)
        inertial = open(os.path.join(CSRC, name)).read()
        assert "& ~(size_t)255" not in inertial and "blkIndex[(size_t)bi *" not in inertial, name
        assert "carve-up overflow" not in inertial and not re.search(r"\breserve\b", inertial), name
        for gone in ("dalloc", "upHi", "stageCap", "cleanup", "arenaBytes"):
            assert not re.search(r"\b%s\b" % gone, inertial), (name, gone)
