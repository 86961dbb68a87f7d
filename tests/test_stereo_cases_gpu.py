"""ComputeStereoMatches on the constructed cases of stereo_cases.py: the mid-scan flush of k_stereo_match, the global-memory form of
k_stereo_median, the un-banded scan, the band limit, and the Hamming / SAD / geometry gates at equality.  mvuRight and mvDepth are compared
with the oracle as float32 bit patterns; rows from a frame's count to the capacity must hold -1.  What path each case takes is asserted in
test_matcher_cases_cpu.py; here every case is checked for legality first (an illegal keypoint would make the SAD stage read outside the
stored pyramid) and the path claims the run depends on are repeated."""
import numpy as np
import pytest

import stereo_cases as S

pytestmark = pytest.mark.gpu

_ORACLE, _EXTRACTED = {}, {}


def _oracle(case):
    if case["name"] not in _ORACLE:
        _ORACLE[case["name"]] = {f: S.oracle_matches(case, f) for f in case["frames"]}
    return _ORACLE[case["name"]]


def _extractor(case):
    """An extractor that has processed the case's 2 * nframes images (left = 2 f, right = 2 f + 1): the stereo matcher reads its pyramid."""
    import torch
    from morb_slam_amd import ORBextractor
    first = case["frames"][min(case["frames"])]
    key = (tuple(sorted((f, id(fr["imgL"]), id(fr["imgR"])) for f, fr in case["frames"].items())), case["nframes"], case["ext"])
    if key not in _EXTRACTED:
        imgs = np.stack([case["frames"].get(f, first)["img" + s] for f in range(case["nframes"]) for s in "LR"])
        ext = ORBextractor(*case["ext"])
        ext.extract_batch(torch.from_numpy(imgs).cuda())
        torch.cuda.synchronize()
        _EXTRACTED.clear()               # one batch of pyramids alive at a time
        _EXTRACTED[key] = ext
    return _EXTRACTED[key]


def run_case(case):
    import torch
    from morb_slam_amd import ORBmatcher
    assert S.legal(case)
    nf, cap = case["nframes"], case["cap"]
    kps = np.zeros((2 * nf, cap), S.KP_DTYPE); desc = np.zeros((2 * nf, cap, 32), np.uint8); cnt = np.zeros(2 * nf, np.int32)
    for f, fr in case["frames"].items():
        for s, side in enumerate("lr"):
            n = len(fr["k" + side])
            kps[2 * f + s, :n] = fr["k" + side]; desc[2 * f + s, :n] = fr["d" + side]; cnt[2 * f + s] = n
    ext = _extractor(case)
    dk = torch.from_numpy(kps.view(np.uint8).reshape(2 * nf, cap, 28)).cuda()
    u, d = ORBmatcher().ComputeStereoMatches(ext, dk, torch.from_numpy(desc).cuda(), torch.from_numpy(cnt).cuda(), case["mbf"], case["mb"])
    torch.cuda.synchronize()
    u, d = u.cpu().numpy(), d.cpu().numpy()
    ora = _oracle(case)
    for f in range(nf):
        n = int(cnt[2 * f])
        if n:
            ue, de = ora[f]
            bad = np.nonzero((u[f, :n].view(np.uint32) != ue.view(np.uint32)) | (d[f, :n].view(np.uint32) != de.view(np.uint32)))[0]
            assert not len(bad), (case["name"], nf, f, bad[:8].tolist(), u[f, bad[:8]].tolist(), ue[bad[:8]].tolist())
        assert (u[f, n:] == -1).all() and (d[f, n:] == -1).all(), (case["name"], nf, f)
    return u, d


@pytest.mark.parametrize("nframes", S.WORKGROUP_SHAPES)
@pytest.mark.parametrize("name", S.EVERY_SHAPE)
def test_every_workgroup_shape(name, nframes):
    """The dense rows and the Hamming thresholds with 1, 2, 4 and 8 left keypoints per wave (1, 3, 9, 33 frames, all but the first empty)."""
    case = S.with_nframes(S.CASES[name](), nframes)
    assert S.legal(case)
    p = S.pairs_per_scan(case, 0)
    if name.startswith("dense"):
        assert p["inside"] >= 1 and p["maxPairs"] <= S.SM_PCAP       # a run cut by a flush in every shape
        if nframes == 33:
            assert p["between"] >= 1
    assert S.sm_lk_for(nframes) == {1: 4, 3: 8, 9: 16, 33: 32}[nframes]
    run_case(case)


def test_median_global():
    case = S.median_global()
    assert S.legal(case)
    assert not S.median_in_regs(case["nframes"], len(case["frames"][0]["kl"]))
    u, _ = run_case(case)
    assert (u[0] >= 0).sum() >= 500


def test_unbanded():
    case = S.unbanded()
    assert S.legal(case)
    assert not S.use_bands(case, 0)
    u, _ = run_case(case)
    assert (u[0] >= 0).sum() >= 10


def test_banded_edge():
    case = S.banded_edge()
    assert S.legal(case)
    assert S.list_total(case, 0) == S.SM_LIST * case["cap"] and S.list_total(case, 1) == S.SM_LIST * case["cap"] + 1
    run_case(case)


@pytest.mark.parametrize("name", ["sad_edges", "few_matches", "geometry_gates"])
def test_gates(name):
    run_case(S.CASES[name]())
