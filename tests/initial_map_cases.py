"""The scenes the initial-map tests share: tests/test_initial_map_gpu.py compares the kernel with the CPU oracle on them,
tests/test_initial_map_cpu.py checks that the oracle's Levenberg-Marquardt path on each of them does not hang on the last bits of a sum
(two builds of the oracle, the points visited in both orders).  A case whose path does is listed in LEFT_OUT and skipped by both."""
import initial_map_oracle as io
from morb_slam_amd.synth import make_initial_map_problem

WIDTH = 256          # csrc/initial_map.hip: IM_T — the threads of a problem's workgroup; a thread owns the points tid, tid + 256, ...
LDS_EDGE = 512       # ... IM_LDS_N — up to this cap the point records live in LDS, beyond it in the handle's workspace
CAP_LDS, CAP_GWS = LDS_EDGE, 832
MIN_TRACKED = 50
CAMS, ROBUST, ITERATIONS = ("pinhole", "kb8"), (1, 0), (0, 1, 5, 20)
# point counts per tier: 49 / 50 straddle minTracked; WIDTH, WIDTH + 1 and 3 WIDTH + 7 exercise the stride loop and the reduction tails; the
# last of each tier fills its cap (every keypoint of both frames is a point)
COUNTS = {CAP_LDS: (8, 49, 50, WIDTH, WIDTH + 1, CAP_LDS), CAP_GWS: (50, 3 * WIDTH + 7, CAP_GWS)}
CASES = [(cam, rob, it, cap, n) for cam in CAMS for rob in ROBUST for it in ITERATIONS for cap, ns in COUNTS.items() for n in ns]
# (cam, robust, iterations, cap, n) whose (iterations, trials) differ between the two oracle builds, or whose outputs differ by more than 1e-6 (a
# hundredth of the parity bar) on the same path: the result turns on the rounding of a sum there
LEFT_OUT = set()

_scenes, _oracle = {}, {}


def scene(cam, cap, n, **kw):
    """One seeded scene per (camera, tier, count): pixel noise of one sigma of the keypoint's level (one edge in twenty is beyond the Huber
    delta, so the robust kernel matters), no gross outliers (TwoViewReconstruction does not triangulate them), points and pose about as far
    from the optimum as a triangulation leaves them.  The cost does not see the scale of the scene, and a start far from the optimum (large
    first steps) lets the scale drift by factors: such a scene amplifies the last bits of every sum and is no test of a kernel."""
    key = (cam, cap, n, tuple(sorted(kw.items())))
    if key not in _scenes:
        full = n == cap
        args = dict(seed=1000 * CAMS.index(cam) + n, n_points=n, cam=cam, noise_px=1.0, outlier_frac=0.0, point_noise=0.01, pose_noise=(0.003, 0.01),
                    baseline=1.0 if cam == "kb8" else 0.4,   # (190 px of focal length: at 0.4 the scale drifts thirtyfold in 20 iterations)
                    n_extra=(0, 0) if full else (20, 15), n_untriangulated=0 if full else 6)
        args.update(kw)
        _scenes[key] = make_initial_map_problem(**args)
    return _scenes[key]


def oracle(key, prob, flags=io.DEFAULT_FLAGS, **kw):
    k = (key, tuple(flags), tuple(sorted(kw.items())))
    if k not in _oracle:
        _oracle[k] = io.run(prob, flags=flags, **kw)
    return _oracle[k]


def case_oracle(case, flags=io.DEFAULT_FLAGS):
    cam, rob, it, cap, n = case
    return oracle(("case",) + tuple(case), scene(cam, cap, n), flags=flags, nIterations=it, robust=rob, depthScale=1.0, minTracked=MIN_TRACKED)


def outlier_scene():
    """Gross outliers and no robust kernel: the first steps overshoot, so the oracle rejects trials (asserted where it is used)."""
    return make_initial_map_problem(seed=72, n_points=120, noise_px=0.5, outlier_frac=0.25, point_noise=0.15, pose_noise=(0.03, 0.1))
