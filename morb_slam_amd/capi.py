"""ctypes binding of libmorb_hip.so, read from include/morb_hip.h (cdecl.py): the signatures, the record layouts and the status codes
have no second copy here.  There is NO CPU fallback: importing this module without the built library, or calling into it without a
GPU, raises."""
import ctypes as C
import os

import numpy as np

from . import cdecl
_DIR = os.path.dirname(os.path.abspath(__file__))
# MORB_HIP_LIB selects another build of the same HIP library (the phase-timing build of tools/fast_phases.py); never a CPU path
LIB_PATH = os.environ.get("MORB_HIP_LIB") or os.path.join(_DIR, "libmorb_hip.so")

HEADER_PATH = os.path.join(os.path.dirname(_DIR), "include", "morb_hip.h")
if not os.path.exists(HEADER_PATH):
    raise ImportError(f"{HEADER_PATH} is missing: the binding (signatures, record layouts, status codes) is read from it")
HEADER = cdecl.parse(open(HEADER_PATH, encoding="utf-8").read(), structures=("morb_frame_params",))   # once per process
KP_DTYPE, FrameParams = HEADER.records["morb_keypoint"], HEADER.structures["morb_frame_params"]
MORB_OK, ERR_INVALID, ERR_HIP, ERR_CAPACITY, ERR_UNSUPPORTED, ERR_EMPTY = (
    HEADER.constants["MORB_" + n] for n in ("OK", "ERR_INVALID", "ERR_HIP", "ERR_CAPACITY", "ERR_UNSUPPORTED", "ERR_EMPTY"))


def make_frame_params(width, height, fx, fy, cx, cy, mbf, mb, scale_factors, level_sigma2, scale_factor=1.2):
    """Frame constructor bookkeeping for an undistorted camera (Frame.cc:229-241, ComputeImageBounds :859-887)."""
    p = FrameParams()
    p.minX, p.minY, p.maxX, p.maxY = 0.0, 0.0, float(width), float(height)
    p.gridInvW = float(np.float32(64.0) / np.float32(p.maxX - p.minX))
    p.gridInvH = float(np.float32(48.0) / np.float32(p.maxY - p.minY))
    p.fx, p.fy, p.cx, p.cy, p.mbf, p.mb = fx, fy, cx, cy, mbf, mb
    p.logScaleFactor = float(np.log(np.float32(scale_factor)))   # mfLogScaleFactor = log(mfScaleFactor) (float)
    p.nlevels = len(scale_factors)
    for i, v in enumerate(scale_factors):
        p.scaleFactors[i] = float(v)
        p.levelSigma2[i] = float(level_sigma2[i])
    return p


def stream_arg(stream):
    """ABI `void* stream` argument.  None = the handle's own HIP stream.  That stream is a blocking stream, i.e. ordered
    with the legacy default stream, but torch may be producing the inputs on a non-default current stream (e.g. the DMA
    of a fresh `.cuda()` upload inside a `torch.cuda.stream(...)` block), so the torch stream is drained first.  Pass a
    raw stream handle (`torch.cuda.Stream.cuda_stream`) to stay asynchronous."""
    if stream is None:
        import torch
        if torch.cuda.is_available():
            torch.cuda.current_stream().synchronize()
        return None
    return C.c_void_p(stream)


class MorbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmorb_hip error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback for the product path)")
        # torch (device memory / streams / torch.distributed plumbing) bundles its own libamdhip64.so.7; load it
        # first so libmorb_hip.so binds to the SAME HIP runtime instead of pulling a second one into the process
        # (two runtimes in one process leave the later one without a GPU).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in HEADER.prototypes.items():   # a declared function the library lacks is an error
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc):
    if rc < 0:
        raise MorbError(rc, lib().morb_last_error().decode(errors="replace"))
    return rc


def ptr(a):
    """Host numpy array or torch tensor (host or device) -> void*."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(a.data_ptr())
