"""Strided and ROI image inputs.  The C ABI takes a row pitch (`stride`) and, batched, an image pitch: a cv::Mat with a step, or a ROI of a larger
frame, is a legal input.  Every input here is a view of a larger POISONED parent buffer (tests/strided_views.py): the pixels of the view are the
synthetic image, every other byte of the parent — row padding, rows above and below, gaps between images — is poison.  The reference for a view is
the CPU oracle on the dense copy of that view; for pyramid level 0 additionally np.pad(view, 19, mode="reflect") (= copyMakeBorder BORDER_REFLECT_101),
which does not depend on the oracle.  Bit-exact everywhere, like tests/test_extractor_gpu.py.

Three one-line mutants that stay inside the caller's buffer were built aside and run once on an MI355X when this file was written:
  * both k_level0 loads with `stride & ~1` (odd strides lose a byte per row): the grid (all three batch sizes), the full-size case, the width
    sweep and the host tests failed (the host entry uploads a dense copy, so an odd width is an odd stride there);
  * k_level0 with `pt.img * stride * height` in place of `pt.img * pitch`: the grid at 3 and 8 images, the full-size case and the poison test failed
    (no earlier test fails: every earlier batch is dense);
  * the selector of the first pad byte of a row one less (register permute only): every test that compares level 0 failed.
What other wrong kernels or host paths would do here, by reading the code (none of these was run; the last two would read out of bounds):
  * k_level0 indexing rows with `width` in place of `stride`: every row but the first is read from the wrong place — rows of poison and shifted
    image bytes — so level 0 differs from np.pad and from the oracle in every grid case with row_pad > 0 (the grid, the width sweep, the full-size case).
  * k_level0 dropping `pt.img * pitch` or using stride * height for it: images 1.. of every case with gap rows / gap bytes read poison or a shifted image.
  * a PyrEdge.sel or PyrEdge.base off by one byte: a pad column of level 0 takes its neighbour's pixel (caught by the np.pad comparison at every width
    whose residue has that edge dword) or, at the right edge, one byte of row padding — then the three poisons give three different level-0 images
    (test_poison_does_not_reach_the_output).
  * an interior 16-byte load one chunk too far right: reads up to 16 bytes behind a row's `width` — poison in every strided case (same test), and
    beyond the allocation in test_views_that_touch_the_ends_of_their_allocation (argued, not provoked).
  * morb_extract copying stride * height bytes: reads stride - width bytes behind the last pixel — the inaccessible page of
    test_host_view_whose_last_pixel_ends_a_mapping."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import procs
from morb_slam_amd.synth import make_image
from strided_views import POISONS, device_view, digest, layout, poison, poisoned_parent

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_HELPER = os.path.join(ROOT, "tests", "native", "extract_view_at_edge.py")

SMALL = (300, 3)          # nfeatures, nlevels of the small images (331 x 120: width mod 4 == 3, (width + 19) mod 16 == 14)
W0, H0 = 331, 120


def _hip(nfeat, nlevels):
    from morb_slam_amd import ORBextractor
    return ORBextractor(nfeat, 1.2, nlevels, 20, 7)


def _oracle(nfeat, nlevels):
    from oracle_lib import OracleExtractor
    return OracleExtractor(nfeat, 1.2, nlevels, 20, 7)


@functools.lru_cache(maxsize=None)
def _expected(w, h, seed, nfeat, nlevels):
    """(image, monoIndex, keypoints, descriptors) of the oracle on the dense synthetic image."""
    img = make_image(w, h, seed=seed)
    return (img,) + _oracle(nfeat, nlevels)(img)


def _extract_view(g, buf, lay):
    """Upload the parent, extract the layout's view through morb_extract_batch; -> (device parent, [(monoIndex, keypoints, descriptors)] per image)."""
    import torch
    from morb_slam_amd import KP_DTYPE
    d_buf = torch.from_numpy(buf).cuda()
    view = device_view(d_buf, lay)
    assert view.data_ptr() == d_buf.data_ptr() + lay.base and view.stride() == (lay.pitch, lay.stride, 1)
    kps, desc, cnt, mono = g.extract_batch(view)
    torch.cuda.synchronize()
    g.check_status()
    cnt = cnt.cpu().numpy(); mono = mono.cpu().numpy(); kps = kps.cpu().numpy(); desc = desc.cpu().numpy()
    return d_buf, [(int(mono[i]), kps[i, :cnt[i]].reshape(-1).view(KP_DTYPE), desc[i, :cnt[i]]) for i in range(lay.nimg)]


def _assert_output(res, exp, what):
    (mono, k, d), (_, mono_o, ko, do) = res, exp
    assert len(k) == len(ko), f"{what}: {len(k)} keypoints, oracle {len(ko)}"
    assert mono == mono_o, f"{what}: monoIndex {mono}, oracle {mono_o}"
    assert k.tobytes() == ko.tobytes(), f"{what}: keypoint records differ"
    np.testing.assert_array_equal(d, do, err_msg=f"{what}: descriptors")


def _assert_stages(g, o, i, what):
    """Every stage tap tests/test_extractor_gpu.py::_compare checks, for image i of the last batch; o has just processed that image."""
    for l in range(g.GetLevels()):
        assert g.level_size(l, i) == o.level_size(l)
        np.testing.assert_array_equal(g.pyramid_level(l, i), o.level_image(l), err_msg=f"{what}: pyramid level {l}")
        co, cg = o.level_candidates(l), g.level_candidates(l, i)
        assert len(co) == len(cg), f"{what}: level {l}: {len(cg)} candidates vs oracle {len(co)}"
        for f in ("x", "y", "response"):
            np.testing.assert_array_equal(cg[f], co[f], err_msg=f"{what}: candidates level {l} field {f}")
        so, sg = o.level_keypoints(l), g.level_keypoints(l, i)
        assert len(so) == len(sg), f"{what}: level {l}: {len(sg)} selected vs oracle {len(so)}"
        for f in ("x", "y", "response", "octave", "size"):
            np.testing.assert_array_equal(sg[f], so[f], err_msg=f"{what}: selected level {l} field {f}")
        bo = o.level_blurred(l)
        if bo is not None:
            np.testing.assert_array_equal(g.blurred_level(l, i), bo, err_msg=f"{what}: blur level {l}")


def _check_case(g, lay, seeds, nfeat, nlevels, kind="random", stages=False, what=""):
    """One view: outputs (and stage taps) against the oracle, level 0 against np.pad, and the caller's buffer unchanged."""
    exp = [_expected(lay.w, lay.h, s, nfeat, nlevels) for s in seeds]
    buf = poisoned_parent(np.stack([e[0] for e in exp]), lay, kind, seed=lay.base + lay.stride)
    d_buf, res = _extract_view(g, buf, lay)
    assert np.array_equal(d_buf.cpu().numpy(), buf), f"{what}: the caller's buffer was written"
    for i in range(lay.nimg):
        _assert_output(res[i], exp[i], f"{what} image {i}")
    for i in (range(lay.nimg) if stages else sorted({0, lay.nimg - 1})):
        np.testing.assert_array_equal(g.pyramid_level(0, i), np.pad(exp[i][0], 19, mode="reflect"), err_msg=f"{what} image {i}: level 0 vs np.pad")
        if stages:
            o = _oracle(nfeat, nlevels)
            o(exp[i][0])
            _assert_stages(g, o, i, f"{what} image {i}")
    return res


@pytest.mark.parametrize("nimg", [1, 3, 8])     # 8: the XCD tile order of py_tile, 3: the plain one
def test_grid_of_views_matches_oracle(nimg):
    """Base offsets 0, 1, 3, 13, 16 (every alignment class of the unaligned 16-byte interior load and of the dword edge load) x row paddings 0 (dense
    rows, shifted base), 1, 3, 37 (odd and even strides) and up to 4096 (a page-multiple stride) x gaps between the images (none, whole rows, rows + 5
    bytes: image_pitch > stride * height, later images at other alignments)."""
    g = _hip(*SMALL)
    seeds = [800 + i for i in range(nimg)]
    gaps = ((0, 0), (2, 0), (1, 5))
    for ip, row_pad in enumerate((0, 1, 3, 37, 4096 - W0)):
        for ix, x0 in enumerate((0, 1, 3, 13, 16)):
            gap_rows, gap_bytes = gaps[(ip + ix) % 3]
            lay = layout(W0, H0, nimg, x0=x0, y0=2, row_pad=row_pad, gap_rows=gap_rows, gap_bytes=gap_bytes)
            assert lay.pitch >= lay.stride * H0 and (row_pad != 4096 - W0 or lay.stride % 4096 == 0)
            _check_case(g, lay, seeds, *SMALL, stages=(x0, row_pad) == (13, 37),
                        what=f"nimg {nimg} x0 {x0} stride {lay.stride} pitch {lay.pitch}")


def test_full_size_view_every_stage():
    """752 x 480 / 1200 features / 8 levels as a view 13 bytes and 3 rows into a parent with rows of 752 + 37 bytes, one row + 5 bytes between the images."""
    lay = layout(752, 480, 3, x0=13, y0=3, row_pad=37, gap_rows=1, gap_bytes=5)
    res = _check_case(_hip(1200, 8), lay, [810, 811, 812], 1200, 8, stages=True, what="752 x 480 view")
    assert all(len(k) > 1000 for _, k, _ in res)


def test_poison_does_not_reach_the_output():
    """The same view with the parent poisoned three ways (0x00, 0xFF, random): outputs and every pyramid level byte-identical across the three, and the
    oracle's.  A kernel that lets one padding byte leak into a pad column of level 0 fails here."""
    g = _hip(*SMALL)
    lay = layout(W0, H0, 3, x0=3, y0=1, row_pad=3, gap_rows=1, gap_bytes=5)
    seeds = [820, 821, 822]
    seen = []
    for kind in POISONS:
        res = _check_case(g, lay, seeds, *SMALL, kind=kind, what=f"{kind} poison")
        seen.append((digest(res), [g.pyramid_level(l, i).tobytes() for i in range(3) for l in range(SMALL[1])]))
    assert seen[0] == seen[1] == seen[2]
    o = _oracle(*SMALL)
    for i, s in enumerate(seeds):
        o(_expected(W0, H0, s, *SMALL)[0])
        assert [o.level_image(l).tobytes() for l in range(SMALL[1])] == seen[0][1][i * SMALL[1]:(i + 1) * SMALL[1]]


def test_sixteen_consecutive_widths_dense_and_strided():
    """The interior / edge split of k_level0 depends on (width + 19) mod 16 and width mod 4: widths 320..335 visit every residue, each as a dense image
    and as a strided view; level 0 against np.pad, all levels and the final output against the oracle."""
    g = _hip(*SMALL)
    for w in range(320, 336):
        for lay in (layout(w, H0), layout(w, H0, x0=13, y0=5, row_pad=37)):
            _check_case(g, lay, [700 + w], *SMALL, stages=True, what=f"width {w} stride {lay.stride}")


def _child_digests(tmp_path, mode):
    r = procs.spawn([sys.executable, EDGE_HELPER, mode], os.environ.copy(), tmp_path / "edge", timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr_tail)
    return dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("DIGEST"))


def _edge_expected(nimg):
    return [_expected(W0, H0, 900 + i, *SMALL)[1:] for i in range(nimg)]     # (the helper's constants: 331 x 120, seeds 900.., 300 features, 3 levels)


@pytest.mark.multiprocess
def test_views_that_touch_the_ends_of_their_allocation(tmp_path):
    """A strided batch whose last pixel is the last byte of a 12 MiB device allocation with a segment of its own, and one whose first pixel is its first
    byte, in a child process (a read beyond the view can fault).  By reading k_level0 no load leaves a row's `width` bytes: interior chunk j loads
    columns [16 j - 19, 16 j - 3) with 16 j - 3 <= width, an edge dword loads [base, base + 4) with 0 <= base <= width - 4."""
    got = _child_digests(tmp_path, "device")
    want = digest(_edge_expected(3))
    assert got == {"end": want, "start": want}


@pytest.mark.multiprocess
def test_host_view_whose_last_pixel_ends_a_mapping(tmp_path):
    """morb_extract on a strided host view whose last pixel is the last accessible byte of a mapping (the next page is PROT_NONE): the host entry reads
    no byte beyond (height - 1) * stride + width.  It copied stride * height bytes before, i.e. stride - width bytes into the next page."""
    assert _child_digests(tmp_path, "host") == {"host": digest(_edge_expected(1))}


def test_strides_the_index_arithmetic_cannot_carry_are_refused():
    """k_level0 forms __umul24(row, stride) + column in 32 bits: stride >= 2^24 or stride * height >= 2^32 would read other rows of the buffer without any
    fault.  Both entries refuse such a stride before anything is launched or copied (so a small real buffer is enough here); a wide parent that the
    arithmetic does carry — a 331 x 120 view in rows of 1 MiB (the extractor takes aspect ratios below 4.5, so not 640 x 120) — passes parity."""
    import torch
    from morb_slam_amd.capi import lib, ptr
    L = lib()
    g = _hip(*SMALL)
    cap = g.max_keypoints
    kps = torch.empty((1, cap, 28), dtype=torch.uint8, device="cuda"); desc = torch.empty((1, cap, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda"); mono = torch.zeros(1, dtype=torch.int32, device="cuda")
    hk = np.zeros((cap, 28), np.uint8); hd = np.zeros((cap, 32), np.uint8); n = C.c_int(0)
    for w, h, stride in ((W0, H0, 1 << 24), (W0, 512, 1 << 23), (W0, H0, (1 << 31) - 1)):
        img = make_image(w, h, seed=830)
        d_img = torch.from_numpy(img).cuda()
        rc = L.morb_extract_batch(g._h, ptr(d_img), 1, w, h, stride, stride * h, None, ptr(kps), ptr(desc), cap, ptr(cnt), ptr(mono), None)
        assert rc in (-1, -4), (stride, h, rc)                     # MORB_ERR_INVALID or MORB_ERR_UNSUPPORTED
        assert b"stride" in L.morb_last_error()
        rc = L.morb_extract(g._h, ptr(img), w, h, stride, 0, 0, ptr(hk), ptr(hd), cap, C.byref(n))
        assert rc in (-1, -4) and n.value == 0, (stride, h, rc)
        assert b"stride" in L.morb_last_error()
    lay = layout(W0, H0, 1, x0=13, y0=1, row_pad=(1 << 20) - W0)
    assert lay.stride == 1 << 20
    _check_case(g, lay, [831], *SMALL, stages=True, what="rows of 1 MiB")


# ---- the host entry: ORBextractor.__call__ -> morb_extract ----

def _host_roi(img, x0, y0, row_pad, kind, seed=0):
    """(parent, ROI): a poisoned 2-D parent with rows of w + row_pad bytes and two rows below the ROI, the image written at (y0, x0)."""
    h, w = img.shape
    assert x0 <= row_pad
    parent = poison((y0 + h + 2) * (w + row_pad), kind, seed).reshape(-1, w + row_pad)
    parent[y0:y0 + h, x0:x0 + w] = img
    return parent, parent[y0:y0 + h, x0:x0 + w]


def test_host_rois_match_oracle():
    """parent[y0:y0+h, x0:x0+w] of a poisoned numpy parent through the host entry: the grid of base offsets and row paddings, each poison, the parent
    unchanged afterwards."""
    g = _hip(*SMALL)
    exp = _expected(W0, H0, 840, *SMALL)
    for row_pad in (16, 19, 37, 4096 - W0):
        for x0 in (0, 1, 3, 13, 16):
            for kind in (POISONS if (x0, row_pad) in ((13, 37), (16, 16)) else ("random",)):
                buf, roi = _host_roi(exp[0], x0, 5, row_pad, kind, seed=x0 + row_pad)
                assert roi.strides == (W0 + row_pad, 1) and not roi.flags.c_contiguous and np.array_equal(roi, exp[0])
                before = buf.copy()
                _assert_output(g(roi), exp, f"host ROI x0 {x0} row_pad {row_pad} {kind} poison")
                np.testing.assert_array_equal(g.pyramid_level(0), np.pad(exp[0], 19, mode="reflect"))
                assert np.array_equal(buf, before)
    exp = _expected(752, 480, 841, 1200, 8)
    buf, roi = _host_roi(exp[0], 13, 3, 37, "random")
    _assert_output(_hip(1200, 8)(roi), exp, "host ROI 752 x 480")


def test_host_views_numpy_can_make_and_the_abi_cannot_take():
    """Negative row stride, pixel step 2, a broadcast row (row stride 0): ORBextractor.__call__ copies them; the result is the oracle's on the dense copy."""
    g = _hip(*SMALL)
    img = make_image(2 * W0, H0, seed=842)
    views = {"flipped rows": img[::-1, :W0], "every second column": img[:, ::2], "broadcast row": np.broadcast_to(img[7, :W0], (H0, W0))}
    assert views["flipped rows"].strides[0] < 0 and views["every second column"].strides[1] == 2 and views["broadcast row"].strides[0] == 0
    for name, v in views.items():
        dense = np.ascontiguousarray(v)
        o = _oracle(*SMALL)
        _assert_output(g(v), (dense,) + o(dense), name)
