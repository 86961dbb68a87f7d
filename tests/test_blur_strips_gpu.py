"""k_blur on linearly numbered strips (csrc/blur_items.h), two output rows per step: every blurred level byte for byte against the CPU
oracle, and the final keypoints and descriptors that are computed from them.  The shapes are the smallest at which the item numbering
and the two-row step can go wrong:

  752 x 480, 8 levels   the bench shape: level 5 (302 x 193) leaves 23 dead rows in its last strip, level 1 (627 px) is no multiple of 8 wide
  333 x 217, 4 levels   odd heights 217, 181, 151, 126: the two-row step ends on an odd row; widths 5 and 6 mod 8
  601 x 377, f = 1.1    other strip counts per row; waves straddle strip rows and levels
  109 x 109, 3 levels   the smallest image configure() accepts with three levels (every level must be at least 76 px: 109, 91, 76);
  91 x 91, 2 levels     ... and with two.  A level of 76 rows ends in a strip of 4 rows, the whole top level is 40 items, and the image's
                        last wave is partly filled.  (A level shorter than one strip cannot be configured; tests/native/blur_items_check.cc
                        covers those in the item mapping.)
  batches of 5 and 8    images of 333 x 217: the plain workgroup order and the XCD order, every image compared
  a batch of one image

The oracle keeps a level's blurred image only if the level has keypoints; it does for every level of every shape here (asserted)."""
import functools

import numpy as np
import pytest

from morb_slam_amd.synth import make_image

pytestmark = pytest.mark.gpu

PARAMS = dict(scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)


@functools.lru_cache(maxsize=None)
def _oracle(w, h, seed, nfeat, scaleFactor, nlevels):
    """The image, its oracle results and the oracle's blurred levels: computed once, shared, never written to."""
    from oracle_lib import OracleExtractor
    img = make_image(w, h, seed=seed)
    o = OracleExtractor(nfeat, scaleFactor, nlevels, PARAMS["iniThFAST"], PARAMS["minThFAST"])
    mono, kps, desc = o(img)
    blurred = [o.level_blurred(l) for l in range(nlevels)]
    sizes = [o.level_size(l) for l in range(nlevels)]
    for a in [img, kps, desc] + [b for b in blurred if b is not None]:
        a.setflags(write=False)
    return img, mono, kps, desc, blurred, sizes


def _gpu(nfeat, scaleFactor, nlevels):
    from morb_slam_amd import ORBextractor
    return ORBextractor(nfeat, scaleFactor, nlevels, PARAMS["iniThFAST"], PARAMS["minThFAST"])


def _check_levels(g, ref, img_index=0):
    _, _, _, _, blurred, sizes = ref
    for l, bo in enumerate(blurred):
        assert g.level_size(l, img_index) == sizes[l]
        assert bo is not None, f"the oracle kept no blurred level {l}"
        np.testing.assert_array_equal(g.blurred_level(l, img_index), bo, err_msg=f"image {img_index} blur level {l}")


SINGLE = [(752, 480, 1, 1200, 1.2, 8), (333, 217, 22, 300, 1.2, 4), (601, 377, 55, 500, 1.1, 6), (109, 109, 7, 200, 1.2, 3), (91, 91, 8, 200, 1.2, 2)]


@pytest.mark.parametrize("w,h,seed,nfeat,f,L", SINGLE, ids=[f"{c[0]}x{c[1]}_L{c[5]}" for c in SINGLE])
def test_blurred_levels_and_descriptors_match_the_oracle(w, h, seed, nfeat, f, L):
    ref = _oracle(w, h, seed, nfeat, f, L)
    img, mono_o, ko, do = ref[:4]
    g = _gpu(nfeat, f, L)
    mono_g, kg, dg = g(img)
    _check_levels(g, ref)
    assert mono_g == mono_o and len(kg) == len(ko)
    assert kg.tobytes() == ko.tobytes(), "keypoint records differ"
    np.testing.assert_array_equal(dg, do)


@pytest.mark.parametrize("nimg", [5, 8, 1])
def test_batches_in_plain_and_xcd_order(nimg):
    import torch
    from morb_slam_amd import KP_DTYPE
    refs = [_oracle(333, 217, 22 + i, 300, 1.2, 4) for i in range(nimg)]
    g = _gpu(300, 1.2, 4)
    imgs = np.stack([r[0] for r in refs])
    kps, desc, cnt, mono = g.extract_batch(torch.from_numpy(imgs).cuda())
    torch.cuda.synchronize()
    cnt = cnt.cpu().numpy(); mono = mono.cpu().numpy(); kps = kps.cpu().numpy(); desc = desc.cpu().numpy()
    for i, ref in enumerate(refs):
        _check_levels(g, ref, i)
        _, mo, ko, do = ref[:4]
        assert cnt[i] == len(ko) and mono[i] == mo
        assert kps[i, :cnt[i]].reshape(-1).view(KP_DTYPE).tobytes() == ko.tobytes()
        np.testing.assert_array_equal(desc[i, :cnt[i]], do)
