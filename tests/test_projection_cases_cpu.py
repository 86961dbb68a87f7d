"""The constructed projection cases (projection_cases.py) under the CPU oracle alone: every builder reached its threshold (it asserts so while it
builds), the oracle's outcome is the one written by hand from the reference lines, and the two sides of every threshold differ."""
import numpy as np
import pytest

import projection_cases as PC


def _ids(entry):
    return [p["name"] for p in PC.problems(entry)]


def _problems(entry):
    return [pytest.param(p, id=p["name"]) for p in PC.problems(entry)]


def _check(p, o):
    print(p["name"], "classes:", p["classes"], "threshold pairs:", len(p["differ"]))
    np.testing.assert_array_equal(o["table"], p["expect"], err_msg=p["name"])
    a = PC.assigned(p, o["table"])
    for x, y in p["differ"]:
        assert a[x] != a[y], (p["name"], "rows %d and %d lie on the two sides of a threshold and came out alike" % (x, y))


@pytest.mark.parametrize("p", _problems("frustum"))
def test_frustum(p):
    o = PC.oracle(p)
    t = o["trk"]
    print(p["name"], "classes:", p["classes"], "threshold pairs:", len(p["differ"]))
    np.testing.assert_array_equal(t["inView"], p["expect"], err_msg=p["name"])
    for i, lv in p["level"].items():
        assert t["level"][i] == lv, (p["name"], i, t["level"][i], lv)
    for i, (u, v) in p["proj"].items():
        assert t["projX"][i] == u and t["projY"][i] == v, (p["name"], i)
    for i in p["nan_rows"]:
        assert np.isnan(t["projX"][i]) and np.isnan(t["projY"][i]) and t["inView"][i] == 1
    for i in np.flatnonzero(p["expect"] == 0):       # a point that fails a test keeps -1 in the fields the failed test comes before
        assert t["level"][i] == -1 and t["depth"][i] == -1 and t["viewCos"][i] == -1 and t["projXR"][i] == -1
    for x, y in p["differ"]:
        assert (t["inView"][x], t["level"][x]) != (t["inView"][y], t["level"][y]), (p["name"], x, y)


def test_predict_scale_boundaries_of_exact_powers():
    """Scale factor 2.0: the boundaries found by bisection are powers of two up to the rounding of logf and of the quotient; whichever side 2^n falls
    on, the next float up predicts the next level."""
    p = [q for q in PC.problems("frustum") if q["name"] == "predict_scale_p20"][0]
    assert len(p["bounds"]) == 2 and p["bounds"][0] == 1.0
    assert abs(float(p["bounds"][1]) / 2.0 - 1.0) < 1e-6
    assert PC.predict_level("p20", p["bounds"][1]) == 1 and PC.predict_level("p20", PC.up(p["bounds"][1])) == 2


@pytest.mark.parametrize("entry", ["mps", "last", "kf", "fuse", "sim3", "init", "tri"])
def test_search_cases(entry):
    for p in PC.problems(entry):
        _check(p, PC.oracle(p))


def test_fuse_gate_sides_differ():
    """The two float32 neighbours of 5.99 and of 7.8 are separate one-point frames: the lower one is fused, the upper one is not."""
    by = {p["name"]: PC.oracle(p)["table"] for p in PC.problems("fuse")}
    for k in ("mono", "stereo"):
        assert by["fuse_gate_%s_lo_fuse" % k][0] == 0 and by["fuse_gate_%s_hi_fuse" % k][0] == -1


def test_search_by_sim3():
    p = PC.problems("sim3dir")[0]
    o = PC.oracle(p)
    np.testing.assert_array_equal(o["v1"], p["expect1"]); np.testing.assert_array_equal(o["v2"], p["expect2"])
    np.testing.assert_array_equal(o["table"], p["expect12"])
    assert (o["v1"] >= len(p["A"]["k"])).any()          # a vnMatch1 entry beyond the OTHER keyframe's count (the agreement kernel reads vn2 there)
    assert ((o["v1"] >= 0) & (o["table"] < 0)).sum() >= 3   # one-sided and disagreeing matches
    for x, y in p["differ"]:
        assert (o["v1"][x] >= 0) != (o["v1"][y] >= 0)


def test_nan_queries_match_nothing():
    p = [q for q in PC.problems("mps") if q["name"] == "mps_th1"][0]
    o = PC.oracle(p)
    bad = np.flatnonzero(~np.isfinite(p["q"]["projX"]) | ~np.isfinite(p["q"]["projY"]))
    assert len(bad) == 6 and not np.isin(o["table"], bad).any()


def test_every_required_class_is_present():
    c = PC.class_counts()
    print("sub-cases per class:", dict(sorted(c.items())))
    for need in ("mps.window", "mps.grid_rounding", "mps.acceptance", "mps.ratio", "mps.ties", "last.rotation_histogram", "frustum.predict_scale",
                 "init.rotation_histogram", "tri.rotation_histogram", "kf.rotation_histogram"):
        assert c.get(need, 0) > 0, need
    for e in PC.ENTRIES:
        for p in PC.problems(e):
            for key in ("k", "k1", "k2"):
                assert len(p.get(key, ())) <= 128
