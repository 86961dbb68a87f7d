"""The pyramid is stored with the three border pixels the blur reads instead of the reference's nineteen (csrc/pyramid_layout.h).
These tests run the extraction at shapes where that layout can go wrong, against the CPU oracle, byte for byte:
  * 314 x 273: level 0 is 320 bytes wide with its pad — a multiple of 64, no slack behind a row — so the wide loads of the blur,
    FAST and the resize run into the next row, the next image and the next level; level 7 is the smallest legal level (76 px);
    315 x 274 and 313 x 275 have ragged dword and row-group ends;
  * scale factor 2.0 (the gather form of the resize) and 1.1;
  * the stereo SAD, which addresses the pyramid from the matcher's translation unit;
  * 65 images in one call (above the team launch's limit), the last image's last level ending the buffer.
The 38-px-padded level the tap returns is the stored block in the middle and a reflected ring around it: it is compared with the
oracle's copyMakeBorder AND with numpy's reflection of its own interior."""
import numpy as np
import pytest

import oracle_lib as O
from morb_slam_amd.synth import make_image, make_stereo_pair

pytestmark = pytest.mark.gpu

NFEAT = 500


def _batch_against_oracle(imgs, scaleFactor=1.2, nlevels=8):
    import torch
    from morb_slam_amd import KP_DTYPE, ORBextractor
    g = ORBextractor(NFEAT, scaleFactor, nlevels, 20, 7)
    kps, desc, cnt, mono = g.extract_batch(torch.from_numpy(np.stack(imgs)).cuda())
    torch.cuda.synchronize()
    g.check_status()
    kps, desc, cnt, mono = kps.cpu().numpy(), desc.cpu().numpy(), cnt.cpu().numpy(), mono.cpu().numpy()
    total = 0
    for i, img in enumerate(imgs):
        o = O.OracleExtractor(NFEAT, scaleFactor, nlevels, 20, 7)
        mono_o, ko, do = o(img)
        for l in range(nlevels):
            assert g.level_size(l, i) == o.level_size(l)
            w, h = o.level_size(l)
            assert w >= 76 and h >= 76
            got = g.pyramid_level(l, i)
            np.testing.assert_array_equal(got, o.level_image(l), err_msg=f"image {i} pyramid level {l}")
            np.testing.assert_array_equal(got, np.pad(got[19:-19, 19:-19], 19, mode="reflect"), err_msg=f"image {i} level {l} border")
            bo = o.level_blurred(l)
            if bo is not None:
                np.testing.assert_array_equal(g.blurred_level(l, i), bo, err_msg=f"image {i} blur level {l}")
            so, sg = o.level_keypoints(l), g.level_keypoints(l, i)
            assert len(so) == len(sg), f"image {i} level {l}: {len(sg)} selected vs oracle {len(so)}"
            for f in ("x", "y", "response", "octave", "size"):
                np.testing.assert_array_equal(sg[f], so[f], err_msg=f"image {i} selected level {l} field {f}")
        assert cnt[i] == len(ko) and mono[i] == mono_o, f"image {i}"
        assert kps[i, :cnt[i]].reshape(-1).view(KP_DTYPE).tobytes() == ko.tobytes(), f"image {i}: keypoint records differ"
        np.testing.assert_array_equal(desc[i, :cnt[i]], do, err_msg=f"image {i} descriptors")
        total += len(ko)
    return total


@pytest.mark.parametrize("w,h", [(314, 273), (315, 274), (313, 275)])
def test_three_images_without_row_slack_match_the_oracle(w, h):
    n = _batch_against_oracle([make_image(w, h, seed=700 + w + k) for k in range(3)])
    assert n > 3 * 200   # the images really give keypoints on every path


@pytest.mark.parametrize("w,h,scaleFactor,nlevels", [(378, 307, 2.0, 3), (314, 273, 1.1, 8)])
def test_other_scale_factors_match_the_oracle(w, h, scaleFactor, nlevels):
    n = _batch_against_oracle([make_image(w, h, seed=800 + k) for k in range(3)], scaleFactor, nlevels)
    assert n > 3 * 200


def test_stereo_matches_on_the_narrow_pad():
    import torch
    from morb_slam_amd import KP_DTYPE, ORBextractor, ORBmatcher
    mbf, mb = np.float32(458.654 * 0.11), np.float32(0.11)
    left, right = make_stereo_pair(314, 273, seed=91)
    ext = ORBextractor(NFEAT, 1.2, 8, 20, 7)
    kps, desc, cnt, _ = ext.extract_batch(torch.from_numpy(np.stack([left, right])).cuda())
    u, d = ORBmatcher().ComputeStereoMatches(ext, kps, desc, cnt, mbf, mb)
    torch.cuda.synchronize()
    ol, orr = O.OracleExtractor(NFEAT), O.OracleExtractor(NFEAT)
    _, kl, dl = ol(left)
    _, kr, dr = orr(right)
    c = cnt.cpu().numpy()
    assert kps[0, :c[0]].cpu().numpy().reshape(-1).view(KP_DTYPE).tobytes() == kl.tobytes()
    assert kps[1, :c[1]].cpu().numpy().reshape(-1).view(KP_DTYPE).tobytes() == kr.tobytes()
    ue, de = O.stereo_matches(ol, orr, kl, dl, kr, dr, mbf, mb)
    n = len(kl)
    assert u[0, :n].cpu().numpy().view(np.uint32).tolist() == ue.view(np.uint32).tolist()
    assert d[0, :n].cpu().numpy().view(np.uint32).tolist() == de.view(np.uint32).tolist()
    assert int((ue >= 0).sum()) > 50   # the SAD refinement really ran


def test_batch_of_65_equals_one_image_calls():
    import torch
    from morb_slam_amd import ORBextractor
    base = [make_image(314, 273, seed=950 + k) for k in range(3)]
    one = ORBextractor(NFEAT, 1.2, 8, 20, 7)
    ref, top = [], []
    for img in base:
        out = one.extract_batch(torch.from_numpy(np.stack([img])).cuda())
        torch.cuda.synchronize()
        ref.append([t.cpu().numpy()[0] for t in out])
        top.append(one.pyramid_level(7, 0))
    many = ORBextractor(NFEAT, 1.2, 8, 20, 7)
    kps, desc, cnt, mono = many.extract_batch(torch.from_numpy(np.stack([base[i % 3] for i in range(65)])).cuda())
    torch.cuda.synchronize()
    many.check_status()
    kps, desc, cnt, mono = kps.cpu().numpy(), desc.cpu().numpy(), cnt.cpu().numpy(), mono.cpu().numpy()
    for i in range(65):
        rk, rd, rc, rm = ref[i % 3]
        assert cnt[i] == rc and mono[i] == rm and rc > 200, f"image {i}"
        assert kps[i, :rc].tobytes() == rk[:rc].tobytes(), f"image {i}: keypoint records differ"
        np.testing.assert_array_equal(desc[i, :rc], rd[:rc], err_msg=f"image {i} descriptors")
    np.testing.assert_array_equal(many.pyramid_level(7, 64), top[64 % 3])   # the block that ends the buffer
    np.testing.assert_array_equal(many.pyramid_level(0, 63), one_level0(base[63 % 3]))


def one_level0(img):
    return np.pad(img, 19, mode="reflect")
