"""Tracking::UpdateLocalMap on the GPU (morb_update_local_map_batch, morb_gather_local_map_points_batch) against the CPU oracle
(tests/native/local_map_oracle.cc) on the cases of tests/local_map_corpus.py.  The path is integer only, so every output is compared
for EQUALITY: both lists with their counts and their -1 padding, pKFmax, the cleared frame table, d_frameLocal, the votes, the
overflow bits.  TrackLocalMapChain is compared with the existing kernels fed with the oracle's local map gathered on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

import local_map_corpus as corpus
import local_map_oracle as oracle
from morb_slam_amd import ORBmatcher
from morb_slam_amd.capi import ERR_INVALID, MORB_OK, lib, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("localKf", "nLocalKf", "refKf", "localMp", "nLocalMp", "frameLocal", "votes", "overflow")


@pytest.fixture(scope="module")
def m():
    o = ORBmatcher(0.8, True)
    yield o
    o.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_tables = {}


def tables(name):
    """A case's map tables on the device, uploaded once per module."""
    if name not in _tables:
        _tables[name] = ORBmatcher.local_map_tables(corpus.get(name)[0], DEV)
    return _tables[name]


def run(m, name, kf_out, mp_cap, queries=None, want_frame_local=True, want_votes=True):
    """-> dict of host arrays: the outputs and frameMp behind the call."""
    s, inertial = corpus.get(name)
    q = slice(None) if queries is None else list(queries)
    frame = _dev(s["frameMp"][q].astype(np.int32))
    out = m.update_local_map(tables(name), frame, _dev(s["count"][q].astype(np.int32)), _dev(s["lastKf"][q].astype(np.int32)), inertial,
                             kf_out=kf_out, mp_cap=mp_cap, want_frame_local=want_frame_local, want_votes=want_votes)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    got["frameMp"] = frame.cpu().numpy()
    return got


def same(got, want, tag, keys=OUTPUTS + ("frameMp",)):
    for k in keys:
        if k in got:
            assert np.array_equal(got[k], want[k]), (tag, k, np.argwhere(got[k] != want[k])[:5], got[k].ravel()[:12], want[k].ravel()[:12])


@pytest.mark.parametrize("name", corpus.SMALL)
def test_equals_the_oracle(m, name):
    """Every small case, the whole batch in one call with capacities a little above the true lengths: base (60 keyframes in a shuffled
    d_kfOrder, four frames), base_inertial (row order, the tail), and one case per quirk; the CPU suite checks on the oracle's results that
    each quirk case shows its quirk (test_the_corpus_reaches_every_rule)."""
    s, inertial = corpus.get(name)
    e = oracle.expected(s, inertial)
    want = oracle.expected(s, inertial, kf_out=e["kf_out"] + 3, mp_cap=e["mp_cap"] + 5)
    got = run(m, name, want["kf_out"], want["mp_cap"])
    same(got, want, name)
    assert not got["overflow"].any()


def test_tie_for_reference_goes_to_the_first_in_order(m):
    got = run(m, "tie_for_reference", 8, 16)
    assert got["votes"][0, 1] == got["votes"][0, 4] == 3 and got["refKf"][0] == 4 and list(got["localKf"][0, :3]) == [4, 2, 1]


def test_bad_top_voter_is_neither_listed_nor_reference_nor_stamped(m):
    got = run(m, "bad_top_voter", 8, 16)
    n = got["nLocalKf"][0]
    assert got["votes"][0, 0] == 5 and got["refKf"][0] == 1 and 0 not in got["localKf"][0, :n] and list(got["localKf"][0, :n]) == [1, 2, 3]


def test_bad_frame_points_are_cleared(m):
    got = run(m, "bad_point_cleared", 8, 16)
    assert list(got["frameMp"][0]) == [0, -1, 1, -1, -1] and list(got["localKf"][0, :got["nLocalKf"][0]]) == [0, 1]


def test_stamped_neighbour_child_and_parent_are_passed_over(m):
    got = run(m, "already_stamped", 8, 16)
    assert list(got["localKf"][0, :got["nLocalKf"][0]]) == [0, 1, 2, 3, 4, 5]


def test_bad_parent_is_added(m):
    got = run(m, "bad_parent_added", 8, 16)
    assert list(got["localKf"][0, :got["nLocalKf"][0]]) == [1, 0] and list(got["localMp"][0, :got["nLocalMp"][0]]) == [4, 5, 0, 1]


def test_parent_ends_the_loop_on_the_first_entry(m):
    got = run(m, "parent_ends_loop", 8, 16)
    assert list(got["localKf"][0, :got["nLocalKf"][0]]) == [1, 2, 3, 0]


def test_first_stage_of_81_adds_nothing_and_79_ends_above_80(m):
    a, b = run(m, "first_stage_81", 100, 16), run(m, "first_stage_79", 100, 16)
    assert a["nLocalKf"][0] == 81 and list(a["localKf"][0, :81]) == list(range(81))
    assert b["nLocalKf"][0] == 82 and list(b["localKf"][0, 79:82]) == [79, 80, 81]


def test_the_inertial_tail(m):
    """It stops at a stamped keyframe, after 20 steps, is skipped at 80 entries and without a last keyframe, runs past 80 entries, and is
    off without IMU."""
    lst = lambda g: list(g["localKf"][0, :g["nLocalKf"][0]])
    assert lst(run(m, "tail_stops_at_stamped", 100, 16)) == [5, 8, 7, 6]
    assert lst(run(m, "tail_off_without_imu", 100, 16)) == [5]
    assert lst(run(m, "tail_twenty_steps", 100, 16)) == [0] + list(range(39, 19, -1))
    assert lst(run(m, "tail_skipped_at_80", 100, 16)) == list(range(80))
    assert lst(run(m, "tail_no_last_keyframe", 100, 16)) == [5, 6]
    assert run(m, "tail_runs_past_80", 100, 16)["nLocalKf"][0] == 95


def test_duplicate_point_in_a_row_and_frame_point_outside_the_local_map(m):
    got = run(m, "duplicate_in_row", 8, 16)
    assert list(got["localMp"][0, :got["nLocalMp"][0]]) == [7, 8, 3, 5, 2] and list(got["frameLocal"][0]) == [2, 1]
    got = run(m, "frame_point_outside", 8, 16)
    assert list(got["frameLocal"][0]) == [0, -1, -1, 1]


def test_size_case(m):
    """1500 keyframes, rows of up to 1200 entries, about 100 local keyframes, thousands of local points: every thread-stride loop and every
    LM_WINDOW loop runs more than once (test_size_case_takes_every_loop_past_its_first_trip holds the figures)."""
    s, inertial = corpus.get("size")
    want = oracle.expected(s, inertial, kf_out=160, mp_cap=8192)
    got = run(m, "size", 160, 8192)
    same(got, want, "size")
    assert (got["nLocalKf"] > 80).all() and (got["nLocalMp"] > 1024).all()


@pytest.mark.parametrize("name", ("base", "first_stage_300"))
def test_capacities_one_short(m, name):
    """kfOut and mpCap one below the longest true lengths: the counts are true, the heads are right, the overflow bits say which list, and
    the words behind each buffer keep their guard pattern."""
    s, inertial = corpus.get(name)
    e = oracle.expected(s, inertial)
    kf_out, mp_cap = int(e["nLocalKf"].max()) - 1, int(e["nLocalMp"].max()) - 1
    want = oracle.expected(s, inertial, kf_out=kf_out, mp_cap=mp_cap)
    nq, cap, nkf, G = len(s["count"]), s["cap"], s["nkf"], 0x5a5a5a5a
    sizes = dict(localKf=nq * kf_out, nLocalKf=nq, refKf=nq, localMp=nq * mp_cap, nLocalMp=nq, frameLocal=nq * cap, votes=nq * nkf, overflow=nq)
    guard = 64
    buf = {k: torch.full((n + guard,), G, dtype=torch.int32, device=DEV) for k, n in sizes.items()}
    shape = dict(localKf=(nq, kf_out), localMp=(nq, mp_cap), frameLocal=(nq, cap), votes=(nq, nkf))
    out = {k: buf[k][:n].view(shape.get(k, (nq,))) for k, n in sizes.items()}
    frame = _dev(s["frameMp"].astype(np.int32))
    m.update_local_map(tables(name), frame, _dev(s["count"].astype(np.int32)), _dev(s["lastKf"].astype(np.int32)), inertial, out=out)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert (want["overflow"] & 1).any() and (want["overflow"] & 2).any() and (want["nLocalKf"] > kf_out).any() and (want["nLocalMp"] > mp_cap).any()
    for k in ("nLocalKf", "refKf", "nLocalMp", "frameLocal", "votes", "overflow"):
        assert np.array_equal(got[k], want[k]), (name, k)
    for q in range(nq):
        nk, nm = min(want["nLocalKf"][q], kf_out), min(want["nLocalMp"][q], mp_cap)
        assert np.array_equal(got["localKf"][q, :nk], want["localKf"][q, :nk]) and np.array_equal(got["localMp"][q, :nm], want["localMp"][q, :nm])
        assert (got["localKf"][q, nk:] == G).all() and (got["localMp"][q, nm:] == G).all()      # entries beyond a count are not written
    for k, n in sizes.items():
        assert (buf[k][n:] == G).all().item(), (name, k, "written past its capacity")


def test_batch_equals_single_calls_and_two_calls_give_the_same_bytes(m):
    s, inertial = corpus.get("base")
    e = oracle.expected(s, inertial)
    whole, again = run(m, "base", e["kf_out"], e["mp_cap"]), run(m, "base", e["kf_out"], e["mp_cap"])
    for k in OUTPUTS + ("frameMp",):
        assert whole[k].tobytes() == again[k].tobytes(), k
    for q in range(len(s["count"])):
        one = run(m, "base", e["kf_out"], e["mp_cap"], queries=[q])
        for k in OUTPUTS + ("frameMp",):
            assert np.array_equal(one[k][0], whole[k][q]), (q, k)


def test_nullable_outputs_may_be_null(m):
    s, inertial = corpus.get("base_inertial")
    e = oracle.expected(s, inertial)
    got = run(m, "base_inertial", e["kf_out"], e["mp_cap"], want_frame_local=False, want_votes=False)
    assert "frameLocal" not in got and "votes" not in got
    same(got, e, "nullable")
    t = dict(tables("base_inertial"))
    t.update(kfOrder=None, childStart=None, child=None, parent=None, prevKf=None)     # the nullable tables: row order, no tree, no chain
    s3 = dict(s, kfOrder=None, childStart=None, child=None, parent=None, prevKf=None, lastKf=np.full(len(s["count"]), -1, np.int32))
    want = oracle.expected(s3, inertial)
    frame = _dev(s["frameMp"].astype(np.int32))
    out = m.update_local_map(t, frame, _dev(s["count"].astype(np.int32)), None, inertial, kf_out=want["kf_out"], mp_cap=want["mp_cap"], want_votes=True)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["frameMp"] = frame.cpu().numpy()
    same(got, want, "null tables")
    assert any(len(a["localKf"]) != len(b["localKf"]) for a, b in zip(e["full"], want["full"]))     # the tree and the chain mattered


def _raw(m, nq=1, nkf=4, kfCap=8, nmp=10, cap=3, kfOut=8, mpCap=16, ncovis=0, name="empty_frame", frame=None, outs=None):
    """The C entry with explicit sizes on the empty_frame case's tables -> (status, outs)."""
    t = tables(name)
    i32 = torch.int32
    full = lambda n: torch.full((max(n, 1),), -7, dtype=i32, device=DEV)
    frame = torch.full((max(nq * cap, 1),), -1, dtype=i32, device=DEV) if frame is None else frame
    count = torch.full((max(nq, 1),), max(cap, 0), dtype=i32, device=DEV)
    o = outs or dict(localKf=full(nq * kfOut), nLocalKf=full(nq), refKf=full(nq), localMp=full(nq * mpCap), nLocalMp=full(nq), frameLocal=full(nq * cap),
                     overflow=full(nq))
    rc = lib().morb_update_local_map_batch(m._h, nq, nkf, kfCap, ptr(t["kfMp"]), ptr(t["kfCount"]), ptr(t["kfFlags"]), None, ptr(t["covis"]), ncovis,
                                           ptr(t["childStart"]), ptr(t["child"]), ptr(t["parent"]), ptr(t["prevKf"]), nmp, ptr(t["mpObsStart"]),
                                           ptr(t["mpObsKf"]), ptr(t["mpFlags"]), cap, ptr(frame), ptr(count), None, 1, kfOut, ptr(o["localKf"]),
                                           ptr(o["nLocalKf"]), ptr(o["refKf"]), mpCap, ptr(o["localMp"]), ptr(o["nLocalMp"]), ptr(o["frameLocal"]),
                                           None, ptr(o["overflow"]), None)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def test_argument_refusals_and_empty_calls(m):
    for bad in (dict(nq=-1), dict(nkf=-1), dict(nmp=-1), dict(ncovis=-1), dict(cap=0), dict(kfCap=0), dict(kfOut=0), dict(mpCap=0)):
        rc, o = _raw(m, **bad)
        assert rc == ERR_INVALID, bad
        assert all((v == -7).all() for v in o.values()), bad
    assert lib().morb_update_local_map_batch(None, *([0] * 32), None) == ERR_INVALID          # NULL handle
    rc, o = _raw(m, nq=0)
    assert rc == MORB_OK and all((v == -7).all() for v in o.values())                          # nothing written
    frame = _dev(np.array([0, 1, -1], np.int32))
    for empty in (dict(nkf=0), dict(nmp=0)):                                                    # empty lists written
        rc, o = _raw(m, frame=frame.clone(), **empty)
        assert rc == MORB_OK, empty
        assert o["nLocalKf"][0] == 0 and o["nLocalMp"][0] == 0 and o["refKf"][0] == -1 and o["overflow"][0] == 0 and (o["frameLocal"] == -1).all(), empty
        assert (o["localKf"] == -7).all() and (o["localMp"] == -7).all()
    g = lib().morb_gather_local_map_points_batch
    assert g(None, *([0] * 19), None) == ERR_INVALID
    assert g(m._h, -1, 1, *([None] * 7), 1, *([None] * 9), None) == ERR_INVALID and g(m._h, 1, 1, *([None] * 7), 0, *([None] * 9), None) == ERR_INVALID
    assert g(m._h, 0, 1, *([None] * 7), 1, *([None] * 9), None) == MORB_OK and g(m._h, 1, 0, *([None] * 7), 1, *([None] * 9), None) == MORB_OK
    assert g(m._h, 1, 1, *([None] * 7), 1, *([None] * 9), None) == ERR_INVALID                 # NULL arguments


def test_gather_copies_the_listed_rows_and_leaves_the_rest(m):
    s, inertial = corpus.get("base")
    e = oracle.expected(s, inertial)
    mp_cap = e["mp_cap"] + 7
    t = tables("base")
    frame = _dev(s["frameMp"].astype(np.int32))
    lm = m.update_local_map(t, frame, _dev(s["count"].astype(np.int32)), _dev(s["lastKf"].astype(np.int32)), inertial, kf_out=e["kf_out"], mp_cap=mp_cap)
    nq = len(s["count"])
    src = dict(Pw="mpPw", normal="mpNormal", maxDist="mpMaxD", minDist="mpMinD", mpDesc="mpDesc", isBad="mpIsBad", mpHasObs="mpObserved")
    out = {k: torch.full((nq, mp_cap) + tuple(t[v].shape[1:]), 77, dtype=t[v].dtype, device=DEV) for k, v in src.items()}
    m.gather_local_map_points(t, lm["localMp"], lm["nLocalMp"], out=out)
    torch.cuda.synchronize()
    for q in range(nq):
        n = int(e["nLocalMp"][q])
        rows = e["full"][q]["localMp"]
        for k, v in src.items():
            g = out[k][q].cpu().numpy()
            assert g[:n].tobytes() == np.ascontiguousarray(s[v][rows]).tobytes(), (q, k)      # bit patterns: a copy
            assert (g[n:] == 77).all(), (q, k, "a row beyond the count was written")
    assert (s["mpIsBad"][np.concatenate([f["localMp"] for f in e["full"]])] == 0).all()


def test_chain_equals_the_existing_kernels_on_the_oracles_local_map():
    """TrackLocalMapChain on a make_local_map_scene map whose keyframe rows are extracted features seen from known poses: its match table
    and pose equal those of isInFrustum -> discard -> SearchByProjection(F, MapPoints) -> PoseOptimization run on the ORACLE's local map,
    gathered on the host and uploaded as the per-frame tables those kernels have always taken."""
    from local_map_chain_case import chain_case, reference_run
    case = chain_case(DEV)
    chain = case["chain"]
    try:
        chain.step()
        chain.sync()
        got = dict(frameMP=chain.frameMP.cpu().numpy(), pose=chain.pose.cpu().numpy(), nLocalMp=chain.lm["nLocalMp"].cpu().numpy(),
                   nmLocal=chain.nmLocal.cpu().numpy(), nInl=chain.nInl.cpu().numpy())
        want = reference_run(case, DEV)
    finally:
        chain.close()
    assert np.array_equal(got["nLocalMp"], want["nLocalMp"]) and (got["nLocalMp"] > 100).all()
    assert np.array_equal(got["frameMP"], want["frameMP"]) and np.array_equal(got["nmLocal"], want["nmLocal"]) and (got["nmLocal"] > 20).all()
    assert got["pose"].view(np.uint32).tobytes() == want["pose"].view(np.uint32).tobytes() and np.array_equal(got["nInl"], want["nInl"])
