"""Extractions whose input view touches the end (or the start) of what the caller owns, each in this process of its own: a read beyond the view is a GPU
memory fault (device cases) or a SIGSEGV (host case) that kills the process, which the parent observes as a non-zero exit code.  Prints one line
`DIGEST <case> <sha256>` per case (tests/strided_views.py: digest); the parent compares it with the CPU oracle's.
Usage: python extract_view_at_edge.py device|host
  device: one uint8 tensor of 12 MiB (a multiple of 2 MiB and >= 10 MiB: the caching allocator gives it a segment of its own), a strided batch of
          three images placed so that the last pixel of the last row of the last image is the tensor's last byte; then the same batch placed so
          that its first pixel is the tensor's first byte.
  host:   n + 1 anonymous pages, the last one made inaccessible; a strided view that starts inside a row of its parent and whose last pixel is
          the last accessible byte, through ORBextractor.__call__ -> morb_extract."""
import ctypes
import mmap
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from morb_slam_amd import KP_DTYPE, ORBextractor
from morb_slam_amd.synth import make_image
from strided_views import Layout, digest, extent, host_view, poison

W, H, NIMG, NFEAT, NLEVELS, ROW_PAD = 331, 120, 3, 300, 3, 37     # (the parent test runs the oracle with the same constants)
SEED = 900


def images():
    return np.stack([make_image(W, H, seed=SEED + i) for i in range(NIMG)])


def device_cases():
    import torch
    from strided_views import device_view
    total = 12 << 20
    stride = W + ROW_PAD
    pitch = stride * (H + 5) + 5
    ext = ORBextractor(NFEAT, 1.2, NLEVELS, 20, 7)
    imgs = images()
    for case in ("end", "start"):
        base = total - extent(W, H, NIMG, stride, pitch) if case == "end" else 0
        lay = Layout(W, H, NIMG, base, stride, pitch, total)
        buf = poison(total, "random", seed=1)
        host_view(buf, lay)[...] = imgs
        d_buf = torch.from_numpy(buf).cuda()
        assert d_buf.numel() == total
        view = device_view(d_buf, lay)
        assert view.data_ptr() == d_buf.data_ptr() + base and (case == "start" or base + extent(W, H, NIMG, stride, pitch) == total)
        kps, desc, cnt, mono = ext.extract_batch(view)
        torch.cuda.synchronize()
        ext.check_status()
        cnt = cnt.cpu().numpy(); mono = mono.cpu().numpy(); kps = kps.cpu().numpy(); desc = desc.cpu().numpy()
        res = [(int(mono[i]), kps[i, :cnt[i]].reshape(-1).view(KP_DTYPE), desc[i, :cnt[i]]) for i in range(NIMG)]
        print("DIGEST", case, digest(res), flush=True)
        del view, d_buf


def host_case():
    libc = ctypes.CDLL("libc.so.6", use_errno=True)
    libc.mmap.restype = ctypes.c_void_p
    libc.mmap.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long]
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    libc.munmap.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    page = mmap.PAGESIZE
    stride = W + ROW_PAD
    need = extent(W, H, 1, stride, 0) + 13
    npages = -(-need // page)
    addr = libc.mmap(None, (npages + 1) * page, mmap.PROT_READ | mmap.PROT_WRITE, mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, -1, 0)
    assert addr and addr != ctypes.c_void_p(-1).value, os.strerror(ctypes.get_errno())
    assert libc.mprotect(addr + npages * page, page, 0) == 0, os.strerror(ctypes.get_errno())     # PROT_NONE
    total = npages * page
    buf = np.ctypeslib.as_array((ctypes.c_ubyte * total).from_address(addr))
    buf[:] = poison(total, "random", seed=2)
    lay = Layout(W, H, 1, total - extent(W, H, 1, stride, 0), stride, stride * H, total)
    view = host_view(buf, lay)
    view[...] = images()[:1]
    img = view[0]
    assert img.strides == (stride, 1) and img.ctypes.data + (H - 1) * stride + W == addr + total     # the last pixel is the last accessible byte
    assert (img.ctypes.data - addr) % stride > 0                                                    # and the view starts inside a row of its parent (x0 > 0)
    ext = ORBextractor(NFEAT, 1.2, NLEVELS, 20, 7)
    mono, k, d = ext(img)
    print("DIGEST host", digest([(mono, k, d)]), flush=True)
    del ext, view, img, buf
    libc.munmap(addr, (npages + 1) * page)


if __name__ == "__main__":
    {"device": device_cases, "host": host_case}[sys.argv[1]]()
    print("OK", flush=True)
