"""The seeded corpus of the MLPnPsolver tests (tests/test_mlpnp_solver_cpu.py runs it through the oracle built two ways, tests/
test_mlpnp_solver_gpu.py through the kernel): Pinhole and KannalaBrandt8 at 0 / 30 / 60 / 85 % outliers with N between 40 and 300,
N = 0, every match missing or bad, N < minInliers, N == minInliers (budget 1) with and without a result, a minInliers near N, a small
maxIterations, planar scenes with one world coordinate exactly 0, repeated and identical points, minSet = 8, feature indices beyond
mvKeysUn, and an N beyond the kernel's LDS path.  A seed whose per-iteration counts depend on the oracle's compiler flags
(test_rounding_does_not_move_the_corpus) is replaced here, and the replacement noted beside it."""
from morb_slam_amd.synth import libc_rand, make_mlpnp_problem

CLEAN = dict(outlier_frac=0.0, noise_px=0.0, bad_frac=0.0, unmatched_frac=0.0)
LDS_N = 384   # csrc/mlpnp_solver.hip: MP_LDS_N


def specs():
    s = []
    for k, cam in enumerate(("pinhole", "kb8")):
        for j, of in enumerate((0.0, 0.3, 0.6, 0.85)):
            s.append(dict(n=60 + 70 * j + 25 * k, cam=cam, outlier_frac=of))
    s += [dict(n=300, cam="pinhole", outlier_frac=0.6, epsilon=0.25),                # 60 % outliers a lower epsilon can still solve
          dict(n=260, cam="kb8", outlier_frac=0.5, epsilon=0.3),
          dict(n=200, cam="pinhole", outlier_frac=0.3, noise_px=1.0),
          dict(n=180, cam="kb8", outlier_frac=0.2, noise_px=0.3),
          dict(n=0),                                                                 # N = 0
          dict(n=40, unmatched_frac=1.0),                                            # no match at all
          dict(n=40, bad_frac=1.0),                                                  # every map point bad
          dict(n=8, **CLEAN),                                                        # N < minInliers (10)
          dict(n=10, **CLEAN),                                                       # N == minInliers: budget 1, the post-loop best branch
          dict(n=10, **dict(CLEAN, outlier_frac=0.5)),                               # budget 1, no result
          dict(n=200, min_inliers=150, outlier_frac=0.3, unmatched_frac=0.0, bad_frac=0.0),   # ~140 inliers < minInliers: the whole budget, noMore
          dict(n=150, outlier_frac=0.3, max_iterations=4),                           # a small maxIterations
          dict(n=120, planar=True, outlier_frac=0.2),                                # planar: world z exactly 0
          dict(n=90, planar=True, cam="kb8", outlier_frac=0.0, noise_px=0.2),
          dict(n=100, dup_frac=0.9, outlier_frac=0.2),                               # mostly repeated points
          dict(n=40, identical=True, **CLEAN),                                       # every sample repeats one point
          dict(n=150, min_set=8, outlier_frac=0.2),
          dict(n=160, beyond_frac=0.2, outlier_frac=0.2),                            # i >= mvKeysUn.size()
          dict(n=640, outlier_frac=0.3, unmatched_frac=0.05),                        # N beyond the LDS path
          dict(n=500, cam="kb8", outlier_frac=0.45, epsilon=0.4, unmatched_frac=0.0, bad_frac=0.0)]
    return s


# spec index -> replacement seed.  22 (90 % repeated points): with seed 22 one iteration's sample repeats a point, the normal matrix has
# a two-dimensional null space and which vector Jacobi returns is decided by rounding: the -O3 -ffp-contract=fast build counted 3
# inliers where the -O2 build counted 0.  About half of the seeds of this spec do that; 106 does not, under five builds.
SEEDS = {22: 106}


def problems(seed0=0):
    probs, rands = [], []
    for k, sp in enumerate(specs()):
        probs.append(make_mlpnp_problem(seed=SEEDS.get(k, seed0 + k), **sp))
        p = probs[-1]
        rands.append(libc_rand(2000 + seed0 + k, p["min_set"] * (p["max_iterations"] + 40)))
    return probs, rands
