"""ctypes front of tests/native/new_map_points_oracle.cc, the CPU oracle of LocalMapping::CreateNewMapPoints: compiled into a temporary
directory with g++ -O2 -ffp-contract=off on first use (lib(flags) builds it another way, for the test that rounding does not move the
corpus)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
SRC = os.path.join(_HERE, "native", "new_map_points_oracle.cc")
DEFAULT_FLAGS = ("-O2", "-ffp-contract=off")
OTHER_FLAGS = ("-O3", "-march=native", "-ffp-contract=fast")
_libs = {}


def lib(flags=DEFAULT_FLAGS):
    flags = tuple(flags)
    if flags not in _libs:
        out = os.path.join(tempfile.mkdtemp(prefix="new_map_points_oracle_"), "libnew_map_points_oracle.so")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-o", out, SRC])
        L = C.CDLL(out)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.new_map_points_oracle_status_names.restype = C.c_char_p
        L.new_map_points_oracle_stat_names.restype = C.c_char_p
        L.new_map_points_oracle_triangulate.argtypes = [vp] * 5
        L.new_map_points_oracle_gate.argtypes = [i, vp, vp, f, f]
        L.new_map_points_oracle_decide.argtypes = [vp] * 12
        L.new_map_points_oracle_run.argtypes = [i, vp, vp, vp, vp, i, i] + [vp] * 7 + [i] + [vp] * 7 + [f, i, i, f, vp, vp, i] + [vp] * 9
        L.new_map_points_oracle_run.restype = None
        _libs[flags] = L
    return _libs[flags]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def names(flags=DEFAULT_FLAGS):
    L = lib(flags)
    return (tuple(L.new_map_points_oracle_status_names().decode().strip(",").split(",")),
            tuple(L.new_map_points_oracle_stat_names().decode().strip(",").split(",")))


def triangulate(x_c1, x_c2, Tc1w, Tc2w):
    a = [np.ascontiguousarray(v, np.float32) for v in (x_c1, x_c2, Tc1w, Tc2w)]
    x = np.zeros(3, np.float32)
    ok = lib().new_map_points_oracle_triangulate(*[_p(v) for v in a], _p(x))
    return bool(ok), x


def gate(monocular, Ow1, Ow2, mb2, medianDepthKF2):
    a, b = np.ascontiguousarray(Ow1, np.float32), np.ascontiguousarray(Ow2, np.float32)
    return bool(lib().new_map_points_oracle_gate(1 if monocular else 0, _p(a), _p(b), float(mb2), float(medianDepthKF2)))


def decide(cam6, sides, scaleFactors, levelSigma2, ratioFactor=1.8, thFarPoints=0.0, inertial=False, farPoints=False):
    """One match through the header's nmp_decide.  sides = two dicts: Tcw, Twc (3 x 4), Ow, x, y, octave and optionally rawx, rawy, ur,
    depth, bStereo, cam8 (a KannalaBrandt8 camera).  Returns (status, x3D, stereoFlags)."""
    T, Ow = np.zeros((2, 2, 12), np.float32), np.zeros((2, 3), np.float32)
    f, i, c8 = np.zeros((2, 6), np.float32), np.zeros((2, 3), np.int32), np.zeros((2, 8), np.float32)
    for k, s in enumerate(sides):
        T[k, 0], T[k, 1], Ow[k] = np.asarray(s["Tcw"], np.float32).ravel(), np.asarray(s["Twc"], np.float32).ravel(), s["Ow"]
        f[k] = [s["x"], s["y"], s.get("rawx", s["x"]), s.get("rawy", s["y"]), s.get("ur", -1.0), s.get("depth", -1.0)]
        i[k] = [s["octave"], 1 if s.get("bStereo") else 0, 1 if "cam8" in s else 0]
        c8[k] = s.get("cam8", list(cam6[:4]) + [0, 0, 0, 0])
    a = [np.ascontiguousarray(cam6, np.float32), np.array([ratioFactor, thFarPoints], np.float32),
         np.array([1 if inertial else 0, 1 if farPoints else 0], np.int32), np.ascontiguousarray(scaleFactors, np.float32),
         np.ascontiguousarray(levelSigma2, np.float32), T, Ow, f, i, c8]
    x, fl = np.zeros(3, np.float32), np.zeros(1, np.int32)
    st = lib().new_map_points_oracle_decide(*[_p(v) for v in a], _p(x), _p(fl))
    return int(st), x, int(fl[0])


def empty_tables(nrows, cap, fill=None):
    """Host twins of ORBmatcher.new_map_point_tables; fill = a byte value every table starts from (a sentinel)."""
    t = dict(Xw=np.zeros((nrows, cap, 3), np.float32), normal=np.zeros((nrows, cap, 3), np.float32), maxDist=np.zeros((nrows, cap), np.float32),
             minDist=np.zeros((nrows, cap), np.float32), desc=np.zeros((nrows, cap, 32), np.uint8), img2=np.full((nrows, cap), -1, np.int32),
             idx2=np.full((nrows, cap), -1, np.int32))
    if fill is not None:
        for v in t.values():
            v.view(np.uint8)[...] = fill
    return t


def run(arrays, flags=DEFAULT_FLAGS, tables=None, hasMP=None, row=None, nrows=None):
    """The whole call on host arrays.  arrays: npairs, nimg, cap, img1, img2, count, kps / kpsRaw (KP_DTYPE records [nimg, cap], kpsRaw
    may be None), desc, uRight / depth (or None), nLeft1 / nLeft2 (or None: pinhole), cam6, scaleFactors, levelSigma2, camL8, camR8,
    match12, poses, kf2First, ratioFactor, inertial, farPoints, thFarPoints.  tables / hasMP are updated in place when given.
    Returns dict(status, stats, tables, hasMP)."""
    A = arrays
    npairs, nimg, cap = int(A["npairs"]), int(A["nimg"]), int(A["cap"])
    row = np.arange(npairs, dtype=np.int32) if row is None else np.ascontiguousarray(row, np.int32)
    nrows = npairs if nrows is None else nrows
    t = empty_tables(nrows, cap) if tables is None else tables
    hasMP = np.zeros((nimg, cap), np.uint8) if hasMP is None else hasMP
    status, stats = np.zeros((npairs, cap), np.int32), np.zeros((npairs, 5), np.int32)
    c = {k: (None if A.get(k) is None else np.ascontiguousarray(A[k])) for k in
         ("img1", "img2", "nLeft1", "nLeft2", "count", "kps", "kpsRaw", "desc", "uRight", "depth", "match12", "kf2First")}
    fl = {k: np.ascontiguousarray(A[k], np.float32) for k in ("cam6", "scaleFactors", "levelSigma2", "camL8", "camR8", "poses")}
    assert c["match12"].dtype == np.int32 and c["kf2First"].dtype == np.uint8 and c["kps"].dtype.itemsize == 28
    lib(flags).new_map_points_oracle_run(
        npairs, _p(c["img1"]), _p(c["img2"]), _p(c["nLeft1"]), _p(c["nLeft2"]), nimg, cap, _p(c["count"]), _p(c["kps"]), _p(c["kpsRaw"]),
        _p(c["desc"]), _p(c["uRight"]), _p(c["depth"]), _p(fl["cam6"]), len(fl["scaleFactors"]), _p(fl["scaleFactors"]), _p(fl["levelSigma2"]),
        _p(fl["camL8"]), _p(fl["camR8"]), _p(c["match12"]), _p(fl["poses"]), _p(c["kf2First"]), float(A["ratioFactor"]),
        1 if A["inertial"] else 0, 1 if A["farPoints"] else 0, float(A["thFarPoints"]), _p(status), _p(stats), nrows, _p(row), _p(t["Xw"]),
        _p(t["normal"]), _p(t["maxDist"]), _p(t["minDist"]), _p(t["desc"]), _p(t["img2"]), _p(t["idx2"]), _p(hasMP))
    return dict(status=status, stats=stats, tables=t, hasMP=hasMP)


def arrays_of_scene(scene):
    """morb_slam_amd.synth.make_new_map_points_scene -> the `arrays` of run()."""
    from morb_slam_amd.capi import KP_DTYPE
    nimg, cap = scene["nimg"], scene["cap"]

    def records(xy):
        k = np.zeros((nimg, cap), KP_DTYPE)
        k["x"], k["y"], k["size"], k["octave"] = xy[..., 0], xy[..., 1], 31.0, scene["octave"]
        return k
    stereo = scene["kind"] in ("stereo1", "stereo2")
    c = scene["cam"]
    return dict(npairs=scene["npairs"], nimg=nimg, cap=cap, img1=scene["img1"], img2=scene["img2"], count=scene["count"],
                kps=records(scene["xy"]), kpsRaw=records(scene["xyRaw"]) if stereo else None, desc=scene["desc"],
                uRight=scene["uRight"] if stereo else None, depth=scene["depth"] if stereo else None,
                nLeft1=scene["nLeft"][scene["img1"]].copy() if scene["rig"] else None,
                nLeft2=scene["nLeft"][scene["img2"]].copy() if scene["rig"] else None,
                cam6=np.array([c["fx"], c["fy"], c["cx"], c["cy"], scene["mb"], scene["mbf"]], np.float32), scaleFactors=scene["scaleFactors"],
                levelSigma2=scene["levelSigma2"], camL8=scene["camL8"], camR8=scene["camR8"], match12=scene["match12"], poses=scene["poses"],
                kf2First=scene["kf2First"], ratioFactor=scene["ratioFactor"], inertial=scene["inertial"], farPoints=scene["farPoints"],
                thFarPoints=scene["thFarPoints"])
