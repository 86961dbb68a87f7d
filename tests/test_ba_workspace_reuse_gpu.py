"""The handle's `work` block shared by LocalInertialBA and the one-shot LocalBundleAdjustment: both carve it anew at every call
(csrc/ba_host.h), so a call finds whatever a larger window or the other adjuster left there, at other offsets.  Each must clear what it
expects to find zero (the Schur operands' zero pattern, the keyframe tickets, the LM words, the solver's x)."""
import numpy as np
import pytest

import oracle_lib as orc
from morb_slam_amd.synth import imu_calib_diagonals, make_ba_problem, make_inertial_ba_problem

pytestmark = pytest.mark.gpu


def _inertial_args(n_opt, n_points):
    nga, walk = imu_calib_diagonals()
    p = make_inertial_ba_problem(n_opt=n_opt, seed=0, n_points=n_points)
    pre = np.stack([orc.imu_preintegrate(p["bias"], nga, walk, p["acc"][a:b], p["gyro"][a:b], p["dt"][a:b])
                    for a, b in zip(p["imuStart"][:-1], p["imuStart"][1:])])
    return (p["kfState"], p["kfKind"], p["mpPos"], p["mpClose"], p["eKF"], p["eMP"], p["eObs"], p["eInvSigma2"], p["iKF1"], p["iKF2"], pre,
            p["iRobust"], p["iInfoScale"], p["cam"], p["Tbc12"])


def test_a_reused_workspace_gives_the_bytes_of_a_fresh_one():
    from morb_slam_amd import Optimizer
    from morb_slam_amd.optimizer import local_bundle_adjustment_oneshot
    b = make_ba_problem(8, 3, 500, seed=2)
    big, small = _inertial_args(10, 1500), _inertial_args(4, 400)
    inertial = lambda args: lambda o: o.LocalInertialBA(*args, bLarge=False)
    visual = lambda o: local_bundle_adjustment_oneshot(o, b["kfPose"], b["kfFixed"], b["mpPos"], b["eKF"], b["eMP"], b["eObs"], b["eInvSigma2"], b["cam"])
    calls = [inertial(big), inertial(small), visual, inertial(small)]
    shared = Optimizer(0)
    try:
        for i, call in enumerate(calls):
            got = call(shared)
            fresh = Optimizer(0)
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want) == 4   # keyframe states, points, erase flags, stats
            for x, y in zip(got, want):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), i
    finally:
        shared.close()
