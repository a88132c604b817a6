"""Write and read a pipeline's planes directly (dust_hip_pipeline_plane_device_ptr + hipMemcpy), so that a test can hand a pass any
input it likes. A helper module, not a test."""
import ctypes

import numpy as np

from dust_amd import api


def _hip():
    lib = ctypes.CDLL("libamdhip64.so")
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.hipMemcpy.restype = ctypes.c_int
    return lib


def _shape(pipe, plane):
    dt, ch = api.PLANE_DTYPES[plane]
    return dt, ((pipe.height, pipe.width, ch) if ch > 1 else (pipe.height, pipe.width))


def upload(pipe, plane, array):
    """the whole plane from `array` (the plane's dtype, shape and byte count). Waits for the pipeline's stream first: whatever was
    enqueued has read or written the plane by then."""
    dt, shape = _shape(pipe, plane)
    a = np.ascontiguousarray(array)
    ptr, nbytes = pipe.plane_device_ptr(plane)
    assert a.dtype == dt and a.shape == shape and a.nbytes == nbytes, (a.dtype, a.shape, a.nbytes, nbytes)
    pipe.exposure()
    assert _hip().hipMemcpy(ctypes.c_void_p(ptr), a.ctypes.data_as(ctypes.c_void_p), nbytes, 1) == 0


def download(pipe, plane):
    dt, shape = _shape(pipe, plane)
    out = np.empty(shape, dt)
    ptr, nbytes = pipe.plane_device_ptr(plane)
    assert out.nbytes == nbytes
    pipe.exposure()
    assert _hip().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), nbytes, 2) == 0
    return out


def empty_scene(ctx):
    """a committed scene with nothing in it: every pass that traces finds the sky, a pass that only reads planes runs as ever"""
    scene = api.Scene(ctx)
    scene.commit()
    return scene


class DeviceMemory:
    """caller-owned device memory (hipMalloc), filled from `array`: what a test binds a plane to"""

    def __init__(self, array):
        self._lib = _hip()
        self._lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self._lib.hipFree.argtypes = [ctypes.c_void_p]
        a = np.ascontiguousarray(array)
        self.dtype, self.shape, self.nbytes = a.dtype, a.shape, a.nbytes
        p = ctypes.c_void_p()
        assert self._lib.hipMalloc(ctypes.byref(p), self.nbytes) == 0
        self.ptr = p.value
        assert self._lib.hipMemcpy(ctypes.c_void_p(self.ptr), a.ctypes.data_as(ctypes.c_void_p), self.nbytes, 1) == 0

    def read(self, pipe):
        """the contents, once the pipeline's stream has drained"""
        out = np.empty(self.shape, self.dtype)
        pipe.exposure()
        assert self._lib.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr), self.nbytes, 2) == 0
        return out

    def free(self):
        if self.ptr:
            assert self._lib.hipFree(ctypes.c_void_p(self.ptr)) == 0
            self.ptr = None
