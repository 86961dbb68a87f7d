"""ORB_SLAM3::KeyFrameDatabase in the reference's signatures (include/morb/KeyFrameDatabase.h), driven from C++ with mock KeyFrame /
Frame / Map types (tests/native/keyframe_database_adapter_check.cc): ONE database object in one process takes adds (in a shuffled
order), an erase, a re-add, a clearMap and four detections, two DetectNBestCandidates and two DetectRelocalizationCandidates.  The
keyframe lists of every detection and the six fields the reference writes on every keyframe (stamp, words, score of both kinds, the
scores as bit patterns) after every detection must equal the CPU oracle driven through the same sequence: the scores one detection
leaves are the entry state of the next."""
import os
import subprocess

import numpy as np
import pytest

import keyframe_database_corpus as corpus
import keyframe_database_oracle as oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def _script(scene, queries):
    """(op, args..) tuples.  Keyframe k's mnId is k + 1; frame ids are beyond every keyframe id."""
    n = len(scene["count"])
    rank = scene["db_rank"]
    order = sorted((k for k in range(n) if rank[k] >= 0), key=lambda k: rank[k])
    q0, q1, q2 = int(queries[2]), int(queries[0]), int(queries[3])        # q0 and q2 are outside the database, q1 is in it
    assert rank[q0] < 0 and rank[q2] < 0 and rank[q1] >= 0
    other = int((scene["map_id"][q0] + 1) % scene["nmaps"])
    ops = [("A", k) for k in order]
    ops += [("N", q0, 3), ("R", q1, 10 * n + 1, int(scene["map_id"][q1])),
            ("E", order[3]), ("E", order[10]), ("A", order[3]), ("A", q0),                  # an erase, a re-add (to the end of the order), the query joins
            ("N", q2, 3), ("M", other), ("R", q0, 10 * n + 2, int(scene["map_id"][q0])), ("N", q1, 2)]
    return ops


def test_reference_signature_class_on_gpu(tmp_path):
    exe = str(tmp_path / "keyframe_database_adapter_check")
    libdir = os.path.join(ROOT, "morb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(NATIVE, "mock_ref"), "-I" + os.path.join(NATIVE, "mock_keyframe_database"),
                           "-I" + os.path.join(ROOT, "include", "morb"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", exe,
                           os.path.join(NATIVE, "keyframe_database_adapter_check.cc"), "-L" + libdir, "-lmorb_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    scene, queries = corpus.ties()
    n = len(scene["count"])
    ops = _script(scene, queries)
    bad_maps = sorted(set(scene["map_id"][(scene["flags"] & 2) != 0].tolist()))
    lines = [f"{scene['nmaps']} {n}", " ".join("1" if m in bad_maps else "0" for m in range(scene["nmaps"]))]
    for k in range(n):
        c = int(scene["count"][k])
        cov = [int(r) for r in scene["covis"][k] if r >= 0]
        con = scene["connected"][k].tolist()
        lines.append(" ".join([str(int(scene["map_id"][k])), str(int(scene["flags"][k] & 1)), str(c)] +
                              [f"{int(w)} {float(v).hex()}" for w, v in zip(scene["word"][k, :c], scene["value"][k, :c])] +
                              [str(len(cov))] + [str(r) for r in cov] + [str(len(con))] + [str(r) for r in con]))
    lines.append(str(len(ops)))
    lines += [" ".join(str(a) for a in op) for op in ops]
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    open(fin, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = open(fout).read().split("\n")
    db = oracle.Database(scene, add=False)
    pos, ncand, nstamped = 0, 0, 0
    for op in ops:
        if op[0] == "A":
            db.add(op[1])
        elif op[0] == "E":
            db.erase(op[1])
        elif op[0] == "M":
            db.clear_map(op[1])
        else:
            if op[0] == "N":
                lo, me, _ = db.detect_n_best(op[1], op[2], qid=op[1] + 1)
                want = ["N", len(lo), *lo.tolist(), len(me), *me.tolist()]
            else:
                c, _ = db.detect_reloc(op[1], op[3], qid=op[2])
                want = ["R", len(c), *c.tolist()]
            assert out[pos].split() == [str(x) for x in want], (op, out[pos], want)
            ncand += len(want) - 2
            pos += 1
            (pq, pw, ps), (rq, rw, rs) = db.state(0), db.state(1)
            for k in range(n):
                g = out[pos + k].split()
                got = (int(g[0]), int(g[1]), np.float32(float.fromhex(g[2])), int(g[3]), int(g[4]), np.float32(float.fromhex(g[5])))
                exp = (int(pq[k]), int(pw[k]), ps[k], int(rq[k]), int(rw[k]), rs[k])
                assert got[:2] == exp[:2] and got[3:5] == exp[3:5], (op, k, got, exp)
                assert got[2].tobytes() == exp[2].tobytes() and got[5].tobytes() == exp[5].tobytes(), (op, k, got, exp)
            nstamped += int((pq != 0).sum() + (rq != 0).sum())
            pos += n
    assert out[pos:] == [""] and ncand >= 6 and nstamped >= 4 * 30
