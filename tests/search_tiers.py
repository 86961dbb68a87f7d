"""Python mirror of morb_slam_amd/csrc/search_tier.h: which implementation a window search of projection.hip takes for a frame
capacity `cap` and `qCap` queries per frame (test_search_tier_cpu.py pins the two against each other).
  1: k_search<MODE, true>   grid, candidates and descriptors in LDS
  2: k_search<MODE, false>  descriptors read from global memory through featOf[p]
  3: k_candidates + k_resolve<MODE> / k_best_per_query (the serial replay)
ENTRY_QCAP and entry_tier() add what each C entry passes: its query capacity, and whether it has a k_search form at all."""

GRID_CELLS = 64 * 48
LDS_LIMIT = 150 * 1024
MAX_ITEMS = 65535


def search_lds_bytes(cap, qCap, withDesc):
    capR, qCapR = (cap + 3) & ~3, (qCap + 3) & ~3
    return (4 * (GRID_CELLS + 4) + 4 * GRID_CELLS + 4 * capR + 4 * qCapR + 16 * capR + (32 * capR if withDesc else 0) + 2 * capR * 3 +
            4 * qCapR + 4 * (qCapR + 4) + 4 * qCapR + capR + 4 * capR)


def search_tier(cap, qCap, serialOnly=False):
    if serialOnly or cap > MAX_ITEMS or qCap > MAX_ITEMS or search_lds_bytes(cap, qCap, False) > LDS_LIMIT:
        return 3
    return 1 if search_lds_bytes(cap, qCap, True) <= LDS_LIMIT else 2


# entry -> (query capacity from the frame capacity and the map-point capacity, has a k_search form)
ENTRY_QCAP = {
    "last": (lambda cap, mpCap: cap, True),       # SearchByProjection(CurrentFrame, LastFrame): window_search MODE 0
    "kf": (lambda cap, mpCap: cap, True),         # SearchByProjection(CurrentFrame, KeyFrame): MODE 0 (the rig form is ranged: serial)
    "mps": (lambda cap, mpCap: mpCap, True),      # SearchByProjection(Frame, MapPoints): MODE 1
    "fuse": (lambda cap, mpCap: mpCap, True),     # Fuse, both forms: best_per_query
    "sim3dir": (lambda cap, mpCap: cap, True),    # SearchBySim3, each direction: best_per_query
    "sim3": (lambda cap, mpCap: mpCap, False),    # SearchByProjection(KF, Scw): always k_candidates + k_resolve<0>
    "init": (lambda cap, mpCap: cap, False),      # SearchForInitialization: always k_candidates + k_resolve<2>
}


def entry_tier(entry, cap, mpCap=None, serial=False):
    """The tier `entry` runs at; serial = MORB_SERIAL_RESOLVE set."""
    q, fast = ENTRY_QCAP[entry]
    return search_tier(cap, q(cap, mpCap), serial or not fast)


def frame_cap(nfeatures):
    """ORBextractor's keypoint capacity at 8 levels, sum of max(quota + 3, 16) + 1 (morb_extractor_max_keypoints), when every level's quota is
    13 or more."""
    return nfeatures + 32
