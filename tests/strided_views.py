"""Images as views of a larger buffer whose every other byte is poison (tests/test_strided_input_gpu.py, tests/test_oracle_cpu.py,
tests/native/extract_view_at_edge.py): the layout arithmetic, the poison, and the digest a child process prints for its parent.
A layout is what the C ABI takes: image i starts at base + i * pitch, its rows lie `stride` bytes apart, a row owns `w` bytes."""
import hashlib
from collections import namedtuple

import numpy as np

POISONS = ("zeros", "ones", "random")

Layout = namedtuple("Layout", "w h nimg base stride pitch total")


def layout(w, h, nimg=1, x0=0, y0=0, row_pad=0, gap_rows=0, gap_bytes=0, tail=64):
    """Rows of w + row_pad bytes, the first image y0 rows and x0 bytes into the buffer, gap_rows rows + gap_bytes bytes between two images,
    `tail` bytes behind the last pixel."""
    stride = w + row_pad
    pitch = stride * (h + gap_rows) + gap_bytes
    base = y0 * stride + x0
    return Layout(w, h, nimg, base, stride, pitch, base + extent(w, h, nimg, stride, pitch) + tail)


def extent(w, h, nimg, stride, pitch):
    """Bytes from the first pixel of the first image to the last pixel of the last one, both included."""
    return (nimg - 1) * pitch + (h - 1) * stride + w


def poison(nbytes, kind, seed=0):
    if kind == "zeros":
        return np.zeros(nbytes, np.uint8)
    if kind == "ones":
        return np.full(nbytes, 0xFF, np.uint8)
    assert kind == "random"
    return np.random.default_rng(0xBAD + seed).integers(0, 256, nbytes, dtype=np.uint8)


def host_view(buf, lay):
    """[nimg, h, w] view of the flat uint8 numpy buffer."""
    assert buf.dtype == np.uint8 and buf.ndim == 1 and lay.base + extent(lay.w, lay.h, lay.nimg, lay.stride, lay.pitch) <= buf.size
    return np.lib.stride_tricks.as_strided(buf[lay.base:], (lay.nimg, lay.h, lay.w), (lay.pitch, lay.stride, 1))


def device_view(d_buf, lay):
    """The same view of a flat uint8 torch tensor."""
    import torch
    assert d_buf.dtype == torch.uint8 and d_buf.dim() == 1 and lay.base + extent(lay.w, lay.h, lay.nimg, lay.stride, lay.pitch) <= d_buf.numel()
    return torch.as_strided(d_buf, (lay.nimg, lay.h, lay.w), (lay.pitch, lay.stride, 1), lay.base)


def poisoned_parent(imgs, lay, kind, seed=0, nbytes=None):
    """Flat buffer of lay.total (or nbytes) poison bytes with the images written into the layout's view."""
    buf = poison(lay.total if nbytes is None else nbytes, kind, seed)
    host_view(buf, lay)[...] = imgs
    return buf


def digest(results):
    """sha256 over (count, monoIndex, keypoint records, descriptors) of every image, in order."""
    s = hashlib.sha256()
    for mono, kps, desc in results:
        s.update(np.array([len(kps), mono], np.int32).tobytes())
        s.update(np.ascontiguousarray(kps).tobytes())
        s.update(np.ascontiguousarray(desc).tobytes())
    return s.hexdigest()
