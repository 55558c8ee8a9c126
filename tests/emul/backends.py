"""TEST INFRASTRUCTURE: the two backends of the kernel entry points (harness_entries.hpp), one calling convention.

A test body calls `be.emu_<name>(...)` with numpy arrays where the kernel reads or writes memory:
  * EmulatedBackend (build.py's host library): an array becomes a pointer to its own data;
  * DeviceBackend (build_device.py's gfx950 library): every array is staged through a torch.cuda buffer -- copied in, the entry
    point called (it synchronises the device), every array copied back IN PLACE, so the body reads its results the same way.
`None` is a null pointer, a list / tuple of arrays is a C array of their pointers, anything else (ints, floats, ctypes objects: the
arguments the harness reads on the host) passes unchanged.  Arrays must be C-contiguous; one array passed twice is one buffer.
Attributes that are not entry points (the product's host C ABI the libraries also export, e.g. vp_resample_coeffs) are the raw
ctypes functions: their pointers are host pointers in both backends."""
import ctypes as ct
import os

import numpy as np


class _Entry:
    """one entry point; argtypes / restype go to the ctypes function"""

    def __init__(self, backend, fn):
        self._be, self._fn = backend, fn

    @property
    def argtypes(self):
        return self._fn.argtypes

    @argtypes.setter
    def argtypes(self, v):
        self._fn.argtypes = v

    @property
    def restype(self):
        return self._fn.restype

    @restype.setter
    def restype(self, v):
        self._fn.restype = v

    def __call__(self, *args):
        return self._be._call(self._fn, args)


class _Backend:
    name = None

    def __init__(self, path):
        # never RTLD_GLOBAL: both libraries export the symbols of libvp_hip.so (linked -Bsymbolic)
        self.lib = ct.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
        self.path = path

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        return _Entry(self, fn) if name.startswith("emu_") else fn

    @staticmethod
    def _check(a):
        if not a.flags.c_contiguous:
            raise ValueError("kernel arguments must be C-contiguous arrays")
        return a


class EmulatedBackend(_Backend):
    name = "emu"

    def _call(self, fn, args):
        keep = []

        def conv(a):
            if a is None:
                return None
            if isinstance(a, np.ndarray):
                return ct.c_void_p(self._check(a).ctypes.data)
            if isinstance(a, (list, tuple)):
                arr = (ct.c_void_p * len(a))(*[None if x is None else self._check(x).ctypes.data for x in a])
                keep.append(arr)
                return arr
            return a

        return fn(*[conv(a) for a in args])


class DeviceBackend(_Backend):
    name = "device"

    def __init__(self, path):
        import torch

        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("the device backend needs a GPU")
        torch.cuda.init()
        super().__init__(path)

    def _call(self, fn, args):
        torch = self.torch
        staged = {}     # (data address, bytes) -> (array, device buffer)

        def stage(a):
            self._check(a)
            key = (a.ctypes.data, a.nbytes)
            if key not in staged:
                buf = torch.empty(max(1, a.nbytes), dtype=torch.uint8, device="cuda")
                if a.nbytes:
                    buf[:a.nbytes].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
                staged[key] = (a, buf)
            return staged[key][1].data_ptr()

        keep = []

        def conv(a):
            if a is None:
                return None
            if isinstance(a, np.ndarray):
                return ct.c_void_p(stage(a))
            if isinstance(a, (list, tuple)):
                arr = (ct.c_void_p * len(a))(*[None if x is None else stage(x) for x in a])
                keep.append(arr)
                return arr
            return a

        cargs = [conv(a) for a in args]
        torch.cuda.synchronize()
        r = fn(*cargs)
        torch.cuda.synchronize()
        for a, buf in staged.values():
            if a.nbytes:
                a.reshape(-1).view(np.uint8)[:] = buf[:a.nbytes].cpu().numpy()
        return r


def load(kind):
    """the backend `kind` ("emu" or "device"), its library built first"""
    if kind == "emu":
        import build

        return EmulatedBackend(build.build())
    if kind == "device":
        import build_device

        return DeviceBackend(build_device.build())
    raise ValueError(kind)
