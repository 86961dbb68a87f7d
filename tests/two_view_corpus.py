"""The seeded corpus of the TwoViewReconstruction tests (tests/test_two_view_cpu.py runs it through the oracle built several ways,
tests/test_two_view_gpu.py through the kernel): two frames of 150 to 400 keypoints (n1 != n2, unmatched keypoints among them: Normalize
reads them), 100 to 300 matches, 200 iterations, one problem at 50, one with more matches than the kernel keeps in LDS (LDS_N).

Kinds (morb_slam_amd.synth.make_two_view_problem): general scenes succeed through ReconstructF; small baselines fail on parallax;
heavy outliers, matches moved along their epipolar line, near-pure rotation and ordinary planar scenes fail on nMinGood / nsimilar.
ReconstructH needs SH > SF, and CheckFundamental forgives whatever CheckHomography forgives (the plane's homography H and any epipole e
give the fundamental matrix [e]x H, whose point-to-line distances are never larger than H's point-to-point distances), so no ordinary
planar scene reaches it: 300 exactly planar noise-free seeds all gave RH <= 0.5.  The "corners" kind does: five corners of one plane,
each matched 30 to 40 times at the same frame-1 position (as one corner is, over the pyramid levels) with pixel noise in frame 2.  Eight
matches of five distinct points leave ComputeF21 a null space of four dimensions, its rank-2 enforcement then moves the matrix, and
SF falls below SH.  Seeds are chosen where ReconstructH then succeeds (about one in ten) or fails its second-best rule.  One of
them spreads each corner's matches over 0.1 px (corner_px), so that no two matches coincide and no sample scores NaN; of 120 seeds at
corner_px 0.02 / 0.1 / 0.3 five / one / three succeed through H, and fewer are stable under the oracle's builds.

A seed whose result depends on the oracle's compiler flags (test_rounding_does_not_move_the_corpus) is replaced here, never
tolerated: the corner seeds listed are those of 400 tried that are stable under both builds."""
from morb_slam_amd.synth import libc_rand, make_two_view_problem

LDS_N = 512   # csrc/two_view.hip: TV_LDS_N, the matches a workgroup keeps in LDS


def _sizes(seed):
    n1, n2 = 230 + seed % 5 * 10, 240 + seed % 3 * 10
    return dict(n_matches=150 + seed % 4 * 20, n1=n1, n2=n2 + 7 * (n1 == n2))


def specs():
    s = [dict(kind="general", seed=k, **_sizes(k)) for k in range(6)]
    s += [dict(kind="general", seed=6, n_matches=300, n1=400, n2=380),
          dict(kind="general", seed=7, max_iterations=50, **_sizes(7)),                     # a shorter RANSAC
          dict(kind="general", seed=8, n_matches=LDS_N + 128, n1=760, n2=800),              # beyond the LDS tier
          dict(kind="general", seed=9, sigma=2.0, noise_px=1.0, **_sizes(9))]
    s += [dict(kind="corners", seed=k, noise_px=0.3, outlier_frac=0.0, corner_px=0.0, **_sizes(k)) for k in (71, 78, 116, 146, 219, 251)]   # through H
    s += [dict(kind="corners", seed=32, noise_px=0.3, outlier_frac=0.0, corner_px=0.1, **_sizes(32))]   # through H, no two matches alike
    s += [dict(kind="corners", seed=1, noise_px=0.3, outlier_frac=0.0, corner_px=0.0, **_sizes(1))]   # H: the second-best rule
    s += [dict(kind="small_baseline", seed=k, **_sizes(k)) for k in (0, 4, 6, 10)]          # a clear winner below one degree
    s += [dict(kind="planar", seed=2, **_sizes(2)), dict(kind="planar", seed=3, **_sizes(3)), dict(kind="rotation", seed=2, **_sizes(2)),
          dict(kind="outliers", seed=0, **_sizes(0)), dict(kind="epipolar", seed=1, **_sizes(1)),
          dict(kind="tiny", seed=0, n_matches=8, n1=150, n2=160),                           # exactly eight matches
          dict(kind="tiny", seed=1, n_matches=12, n1=160, n2=150),
          dict(kind="tiny", seed=2, n_matches=5, n1=150, n2=170),                           # fewer than eight: no iteration
          dict(kind="tiny", seed=3, n_matches=0, n1=180, n2=150)]                           # no match at all
    return s


def problems():
    probs, rands = [], []
    for sp in specs():
        probs.append(make_two_view_problem(**sp))
        rands.append(libc_rand(100 + sp["seed"], 8 * probs[-1]["max_iterations"]))
    return probs, rands


def assert_composition(probs, oracle):
    """What the corpus must hold, on the oracle's results: the tests cannot pass on an empty or one-sided corpus."""
    from morb_slam_amd.optimizer import TWO_VIEW_FAIL
    fail = {n: k for k, n in enumerate(TWO_VIEW_FAIL)}
    assert len(probs) >= 24
    assert all(p["n1"] != p["n2"] and (p["matches12"] < 0).any() for p in probs)
    assert sum(1 for o in oracle if o["ok"] and o["MODEL"] == 2) >= 6
    assert sum(1 for p, o in zip(probs, oracle) if o["ok"] and o["MODEL"] == 1 and p["kind"] == "corners") >= 3
    assert sum(1 for o in oracle if not o["ok"] and o["FAIL"] == fail["PARALLAX"]) >= 2
    assert sum(1 for o in oracle if not o["ok"] and o["FAIL"] == fail["AMBIGUOUS"] and o["N"] >= 100) >= 2
    assert any(not o["ok"] and o["FAIL"] == fail["AMBIGUOUS"] and o["MODEL"] == 1 for o in oracle)   # the H second-best rule
    assert any(o["N"] == 8 for o in oracle) and any(0 < o["N"] < 8 for o in oracle) and any(o["N"] == 0 for o in oracle)
    assert all(o["MODEL"] == 0 and o["FAIL"] == fail["FEW_MATCHES"] and not o["ok"] for o in oracle if o["N"] < 8)
    assert any(o["ok"] and o["BEST_IT_H"] > 0 and o["BEST_IT_F"] > 0 for o in oracle)
    assert any(o["N"] > LDS_N and o["ok"] for o in oracle) and any(p["max_iterations"] == 50 for p in probs)
