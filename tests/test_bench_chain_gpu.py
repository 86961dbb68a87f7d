"""The BENCHED chain against the oracle: the exact object bench.py times (morb_slam_amd/frontend.py StereoFrontEnd — two buffer
sets, pipelined streams, the k=10 / L=6 / levelsup=4 vocabulary, the has_mp mask, bench.py's default batch of stereo frames per step) is
run for three steps and sampled frames spread over the batch are compared with the CPU oracle field by field: keypoint records,
descriptors, mvuRight / mvDepth bit patterns, BoW word + node ids, the SearchByBoW table and count (tests/chain_check.py).

Reference: ORBextractor.cc:1006-1086, Frame.cc:889-1047, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1218-1259,
ORBmatcher.cc:218-395."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _front_end(B, **kw):
    import torch
    import bench
    from morb_slam_amd.frontend import StereoFrontEnd
    host = bench.make_batch(list(range(B)), B, seed=0).reshape(2 * B, bench.H, bench.W)
    images = torch.from_numpy(host).cuda()
    return StereoFrontEnd(images, 1200, B, vocab=(10, 6, 4), **kw), host


def test_bench_step_matches_oracle():
    import bench
    import chain_check
    B = bench.WORKLOADS["c2"][3]      # the batch bench.py runs by default (512 stereo frames = 1024 images per launch)
    assert B >= 128
    fe, host = _front_end(B)
    sets = [fe.step() for _ in range(3)]
    fe.sync()
    # step 3 wrote buffer set 0 again (its readers of step 1 were waited for), step 2 wrote set 1: both are checked
    frames = sorted(set(int(x) for x in np.linspace(0, B - 1, 8)) | {1, B // 2 + 1})
    assert chain_check.verify_frames(fe, sets[2], frames, host) == len(frames)
    assert chain_check.verify_frames(fe, sets[1], [0, 37, B - 1], host) == 3
    assert sets[2] is sets[0] and sets[1] is not sets[0]
    nm = sets[2].match_out[1].cpu().numpy()
    assert nm[1:].mean() > 50                     # frames really match their predecessors
    fe.close()


@pytest.mark.parametrize("kw", [dict(matchers="under-quadtree"), dict(matchers="under-fast"), dict(extract_streams=2), dict(nset=1)])
def test_other_schedules_match_oracle(kw):
    """bench.py's other schedules (--matchers under-quadtree | under-fast, --extract-streams 2, --no-pipeline) produce the same bytes."""
    import chain_check
    B = 32
    fe, host = _front_end(B, **kw)
    for _ in range(3):
        S = fe.step()
    fe.sync()
    assert chain_check.verify_frames(fe, S, [0, 13, B - 1], host) == 3
    fe.close()


@pytest.mark.multiprocess
def test_bench_line_reports_verified_frames_and_sustained(tmp_path):
    """bench.py's own post-region self-check and the sustained block (short run)."""
    from procs import describe, spawn
    p = spawn([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "16", "--steps", "3", "--warmup", "1", "--full", "--no-extras",
               "--no-cpu-baseline", "--verify-frames", "3", "--sustained-s", "0.3"], dict(os.environ), tmp_path / "log", timeout=900)
    assert p.returncode == 0, describe([p])
    line = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]
    assert line["verified_frames"] == 3 and line["verified"]["frames"] == [0, 7, 15]
    s = line["sustained"]
    assert s["steps"] >= 1000 and s["window_min"] <= s["window_median"] <= s["window_max"] and s["value"] > 0


@pytest.mark.multiprocess
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps and prints the headline keys only; --dump-outputs writes the last timed step's
    outputs as float .npy files, and the sampled frames in them are the oracle's (keypoints, descriptors, stereo, BoW, SearchByBoW)."""
    import bench
    import oracle_lib as O
    from morb_slam_amd.synth import make_vocabulary
    from procs import describe, spawn
    B = 16
    d = tmp_path / "out"
    p = spawn([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", str(B), "--steps", "4", "--warmup", "1", "--dump-outputs", str(d)],
              dict(os.environ), tmp_path / "log", timeout=900)
    assert p.returncode == 0, describe([p])
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] - B * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
    for k in ("roofline", "sustained", "verified", "cpu_baseline", "extra_metrics", "latency", "h2d_inclusive", "extract_stage_ms_per_step"):
        assert k not in line, k
    a = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    frames = a["frames"].astype(int)
    assert len(frames) == B and list(frames) == list(range(B))
    host = bench.make_batch(list(range(B)), B, seed=0).reshape(2 * B, bench.H, bench.W)
    vd, vf = make_vocabulary(10, 6, seed=0)
    for i in (0, 5, B - 1):
        f = int(frames[i])
        ora = []
        for side in (0, 1):
            o = O.OracleExtractor(1200, 1.2, 8, 20, 7)
            _, ko, do = o(host[2 * f + side])
            n = len(ko)
            assert a["keypoint_count"][2 * f + side] == n
            kp = a["keypoints"][i, side, :n]
            for j, name in enumerate(ko.dtype.names):
                np.testing.assert_array_equal(kp[:, j], ko[name].astype(np.float64), err_msg=f"frame {f} image {side}: {name}")
            assert not a["keypoints"][i, side, n:].any()
            np.testing.assert_array_equal(a["descriptors"][i, side, :n], do.astype(np.float32))
            ora.append((o, ko, do))
        (ol, kl, dl), (orr, kr, dr) = ora
        ue, de = O.stereo_matches(ol, orr, kl, dl, kr, dr, np.float32(458.654 * 0.11), np.float32(0.11))
        n = len(kl)
        assert a["stereo_uright"][i, :n].astype(np.float32).tobytes() == ue.tobytes()
        assert a["stereo_depth"][i, :n].astype(np.float32).tobytes() == de.tobytes()
        we, ne = O.bow_transform(dl, vd, vf, 10, 6, 4)
        np.testing.assert_array_equal(a["bow_word"][i, :n], we.astype(np.float64))
        np.testing.assert_array_equal(a["bow_node"][i, :n], ne.astype(np.float64))
    # SearchByBoW of frame 1 against frame 0 (bench's has_mp mask: StereoFrontEnd's default seed)
    rng = np.random.default_rng(7)
    o0, o1 = O.OracleExtractor(1200, 1.2, 8, 20, 7), O.OracleExtractor(1200, 1.2, 8, 20, 7)
    (_, k0, d0), (_, k1, d1) = o0(host[0]), o1(host[2])
    cap = a["keypoints"].shape[2]
    has_mp = (rng.random((2 * B, cap)) < 0.8).astype(np.uint8)
    _, n0 = O.bow_transform(d0, vd, vf, 10, 6, 4)
    _, n1 = O.bow_transform(d1, vd, vf, 10, 6, 4)
    cnt_e, me = O.search_by_bow(d0, k0["angle"], has_mp[0, :len(k0)], n0, d1, k1["angle"], n1, 0.7, True)
    assert a["search_by_bow_count"][1] == cnt_e and cnt_e > 0
    np.testing.assert_array_equal(a["search_by_bow_match"][1, :len(k1)], me.astype(np.float64))
