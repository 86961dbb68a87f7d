"""The seeded scenes of the KeyFrameDatabase tests (tests/test_keyframe_database_cpu.py runs them through the oracle and a numpy brute
force, tests/test_keyframe_database_gpu.py through the kernels).  Each function returns (scene, queries); a scene is a
morb_slam_amd.synth.make_keyframe_database_scene dict.  The shapes are the smallest at which each part of the kernels can go wrong:
70 keyframes (more than one wave of them, not a multiple of 64 nor of the 4 waves of a workgroup), up to 100 words per keyframe
(more than one pass of 64 lanes), cap 128 > every count."""
import numpy as np

from morb_slam_amd.synth import make_keyframe_database_scene

LDS_N = 4096   # csrc/keyframe_database.hip: MORB_KFDB_LDS_N, the pool size up to which a query's lists stay in LDS
N_CAND = 3


def _queries(scene, nq, seed, in_db):
    """nq query rows with at least 20 words that are not on words of their own: the first `in_db` of them in the database, the
    others not (the usual case: LoopClosing queries a keyframe before it is added).  Each gets a connected set of four."""
    rng = np.random.default_rng(seed)
    rows = [int(r) for r in rng.permutation(len(scene["count"])) if scene["count"][r] >= 20 and scene["word"][r, 0] < scene["nwords_voc"] - 200]
    ins = [r for r in rows if scene["db_rank"][r] >= 0][:in_db]
    rest = [r for r in rows if r not in ins][:nq - len(ins)]
    for r in rest:
        scene["db_rank"][r] = -1
    n = len(scene["count"])
    for r in ins + rest:        # the neighbours on the trajectory, which share the query's place and would head its lists, are connected
        scene["connected"][r] = np.array([k for k in (r - 2, r - 1, r + 1, r + 3) if 0 <= k < n], np.int32)
    return np.array(ins + rest, np.int32)


def base():
    s = make_keyframe_database_scene(seed=1, nKF=70, nwords_voc=1000, words_per_kf=(20, 100), nmaps=2, cap=128, ncovis=10, bad_maps=())
    q = _queries(s, 5, 11, 2)
    return s, q


def base_bad_map():
    """the base scene with map 1 bad: queries of map 0 get no merge candidate, queries of map 1 are unaffected"""
    s = make_keyframe_database_scene(seed=1, nKF=70, nwords_voc=1000, words_per_kf=(20, 100), nmaps=2, cap=128, ncovis=10, bad_maps=(1,))
    q = _queries(s, 5, 11, 2)
    return s, q


def ties():
    s = make_keyframe_database_scene(seed=2, nKF=70, nwords_voc=1000, words_per_kf=(20, 100), nmaps=2, cap=128, ncovis=10, dup_groups=8,
                                     dup_size=5, bad_frac=0.03)
    return s, _queries(s, 5, 12, 2)


def stale():
    s = make_keyframe_database_scene(seed=3, nKF=70, nwords_voc=1000, words_per_kf=(20, 100), nmaps=2, cap=128, ncovis=10, bad_frac=0.0,
                                     erased_frac=0.0)
    return s, _queries(s, 3, 13, 0)


def large():
    s = make_keyframe_database_scene(seed=4, nKF=5000, nwords_voc=20000, words_per_kf=(64, 64), nmaps=2, cap=64, ncovis=10, nplaces=40)
    return s, _queries(s, 2, 14, 1)


def one_word():
    s = make_keyframe_database_scene(seed=5, nKF=70, nwords_voc=6, words_per_kf=(1, 1), nmaps=2, cap=4, ncovis=10, disjoint=0, place_frac=0.0)
    rng = np.random.default_rng(15)
    return s, rng.choice(70, 5, replace=False).astype(np.int32)


def empty_database():
    s, q = base()
    s["db_rank"][:] = -1
    return s, q


def no_shared_word():
    """the queries are the keyframes on words of their own, taken out of the database: nothing shares a word with them"""
    s, _ = base()
    lonely = np.nonzero(s["word"][:, 0] >= s["nwords_voc"] - 200)[0].astype(np.int32)
    assert len(lonely) == 2
    s["db_rank"][lonely] = -1
    return s, lonely


def all_connected():
    s, q = base()
    for r in q:
        s["connected"][int(r)] = np.arange(len(s["count"]), dtype=np.int32)
    return s, q


def all_bad():
    s, q = base()
    s["flags"] |= 1
    return s, q


def hand_scene(vectors, ncovis=2, covis=None):
    """a scene from explicit {word: weight} dicts (weights are L1-normalised here), all in the database in row order"""
    n, cap = len(vectors), max(max((len(v) for v in vectors), default=1), 1)
    word, value, count = np.zeros((n, cap), np.int32), np.zeros((n, cap), np.float64), np.zeros(n, np.int32)
    for k, v in enumerate(vectors):
        ws = sorted(v)
        tot = sum(abs(v[w]) for w in ws)
        word[k, :len(ws)], value[k, :len(ws)], count[k] = ws, [v[w] / tot for w in ws], len(ws)
    cv = np.full((n, ncovis), -1, np.int32)
    for k, row in (covis or {}).items():
        cv[k, :len(row)] = row
    return dict(word=word, value=value, count=count, db_rank=np.arange(n, dtype=np.int32), covis=cv,
                connected=[np.zeros(0, np.int32) for _ in range(n)], map_id=np.zeros(n, np.int32),
                flags=np.zeros(n, np.uint8), nwords_voc=64, nmaps=1, cap=cap, ncovis=ncovis)


def at_threshold():
    """The query (row 0, outside the database) has words 0..9.  Row 1 shares all ten: maxCommonWords = 10, minCommonWords =
    (int)(10 * 0.8f) = 8.  Row 2 shares exactly eight and must NOT be scored; row 3 shares nine and is; row 4 shares one."""
    q = {w: 1.0 + w for w in range(10)}
    v = [q, {w: 2.0 for w in range(10)}, {**{w: 1.5 for w in range(8)}, 20: 1.0, 21: 3.0}, {**{w: 1.0 for w in range(9)}, 22: 2.0},
         {9: 1.0, 30: 1.0, 31: 1.0}]
    s = hand_scene(v, covis={1: [2, 3], 3: [2]})
    s["db_rank"] = np.array([-1, 0, 1, 2, 3], np.int32)
    return s, np.array([0], np.int32)


def stale_neighbour():
    """Two queries in a row on one database.  Rows 0 and 1 are the queries (outside the database).  Query 0 scores rows 2 and 3.
    Query 1 scores row 2 again but only STAMPS row 3 (one common word against ten), and row 3 is a covisibility neighbour of row
    2: row 2's accumulated score takes row 3's score of query 0."""
    q0 = {w: 1.0 for w in range(10)}
    q1 = {**{w: 1.0 for w in range(20, 30)}, 0: 1.0}
    r2 = {**{w: 1.0 for w in range(10)}, **{w: 2.0 for w in range(20, 30)}}
    r3 = {**{w: 3.0 for w in range(10)}, 40: 1.0}
    s = hand_scene([q0, q1, r2, r3], covis={2: [3]})
    s["db_rank"] = np.array([-1, -1, 0, 1], np.int32)
    return s, np.array([0, 1], np.int32)


def reloc_maps(scene, queries):
    """the map each relocalisation query searches: its own keyframe's map, and the other one for every second query, so that entries
    whose best keyframe lies in another map are dropped"""
    m = scene["map_id"][queries].copy()
    m[1::2] = (m[1::2] + 1) % scene["nmaps"]
    return m.astype(np.int32)
