"""Caller-owned HIP streams for the tests of the C ABI's `void *stream` arguments (tests/test_streams_gpu.py): ctypes on the HIP
runtime that the project's shared library is linked against — the object the library itself calls (a process may hold a second HIP
runtime: PyTorch's), found through the library's own symbol resolution and opened again by its soname without loading anything new
(RTLD_NOLOAD).

`delay(stream)` enqueues filler work on a caller's stream: FILLER_REPEATS x hipMemsetAsync over a scratch buffer of FILLER_BYTES that
the helper owns.  Enqueued directly in front of a library call, it keeps everything the library enqueues on that stream waiting, so
whatever the library enqueues on the null stream instead (not ordered against a non-blocking stream), or reads on the host without
waiting for the stream, runs ahead of the stream's work and sees stale data.  The filler is long enough when hipStreamQuery still
answers hipErrorNotReady right after an asynchronous entry point has returned; the tests assert that (DESIGN.md "Streams" has the size
that was needed and how it was found).

A stream must outlive every context that ran on it: close the contexts, then synchronise and destroy the stream (`Streams` does it in
that order when used as the tests use it: contexts are closed inside the `with` block)."""
import ctypes as C
import os
import re

from flagger_amd import _native as N

hipSuccess = 0
hipErrorNotReady = 600
hipStreamDefault = 0
hipStreamNonBlocking = 1

FILLER_BYTES = 256 << 20
FILLER_REPEATS = 16


class HipError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        super().__init__("%s failed with HIP error %d" % (where, code))


class _DlInfo(C.Structure):
    _fields_ = [("dli_fname", C.c_char_p), ("dli_fbase", C.c_void_p), ("dli_sname", C.c_char_p), ("dli_saddr", C.c_void_p)]


def _address(handle: C.CDLL, name: str) -> int:
    return C.cast(getattr(handle, name), C.c_void_p).value


def _runtime_of_the_library() -> C.CDLL:
    """The HIP runtime the project's library calls.  A process may hold more than one (PyTorch ships a copy of its own, and a test
    that imported torch earlier has mapped it): dlsym on the library's own handle searches its dependencies, so the object that defines
    the library's hipStreamQuery is the one — found with dladdr, opened again by its soname (or path) without loading anything, and
    accepted only when it resolves hipStreamQuery to the same address."""
    lib = N.lib()
    want = _address(lib, "hipStreamQuery")
    dl = C.CDLL(None)
    dl.dladdr.restype, dl.dladdr.argtypes = C.c_int, [C.c_void_p, C.POINTER(_DlInfo)]
    info = _DlInfo()
    if not dl.dladdr(C.c_void_p(want), C.byref(info)) or not info.dli_fname:
        raise RuntimeError("the project's library resolves no HIP runtime (hipStreamQuery)")
    path = os.path.realpath(info.dli_fname.decode())
    m = re.search(r"(libamdhip64\.so\.\d+)", os.path.basename(path))
    noload = getattr(os, "RTLD_NOLOAD", 4)
    for name in ([m.group(1)] if m else []) + [info.dli_fname.decode(), path]:
        try:
            rt = C.CDLL(name, mode=noload | os.RTLD_NOW)       # the object already in the process, or nothing
        except OSError:
            continue
        if _address(rt, "hipStreamQuery") == want:
            return rt
    raise RuntimeError("cannot open the HIP runtime the project's library uses (%s)" % path)


class Hip:
    """The few runtime calls the stream tests need; every call checks its return code."""

    def __init__(self):
        rt = _runtime_of_the_library()
        vp, u32, i32, sz = C.c_void_p, C.c_uint, C.c_int, C.c_size_t
        for name, args in (("hipStreamCreateWithFlags", [C.POINTER(vp), u32]), ("hipStreamDestroy", [vp]), ("hipStreamQuery", [vp]),
                           ("hipStreamSynchronize", [vp]), ("hipMalloc", [C.POINTER(vp), sz]), ("hipFree", [vp]),
                           ("hipMemsetAsync", [vp, i32, sz, vp]), ("hipSetDevice", [i32]), ("hipGetLastError", [])):
            fn = getattr(rt, name)
            fn.restype, fn.argtypes = i32, args
        self._rt = rt
        self._scratch = None

    def _ok(self, code, where):
        if code != hipSuccess:
            self._rt.hipGetLastError()
            raise HipError(code, where)

    def set_device(self, device: int = 0):
        self._ok(self._rt.hipSetDevice(device), "hipSetDevice")

    def stream_create(self, non_blocking: bool = True, device: int = 0) -> int:
        self.set_device(device)                         # (the device of the contexts the stream will serve)
        s = C.c_void_p()
        self._ok(self._rt.hipStreamCreateWithFlags(C.byref(s), hipStreamNonBlocking if non_blocking else hipStreamDefault),
                 "hipStreamCreateWithFlags")
        return int(s.value)

    def stream_destroy(self, s: int):
        self._ok(self._rt.hipStreamDestroy(C.c_void_p(s)), "hipStreamDestroy")

    def stream_query(self, s: int) -> int:
        """hipSuccess (everything enqueued has completed) or hipErrorNotReady; anything else raises."""
        code = self._rt.hipStreamQuery(C.c_void_p(s))
        if code not in (hipSuccess, hipErrorNotReady):
            self._ok(code, "hipStreamQuery")
        if code == hipErrorNotReady:
            self._rt.hipGetLastError()                  # (not an error: keep it out of the library's next hipGetLastError)
        return code

    def stream_synchronize(self, s: int):
        self._ok(self._rt.hipStreamSynchronize(C.c_void_p(s)), "hipStreamSynchronize")

    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._ok(self._rt.hipMalloc(C.byref(p), nbytes), "hipMalloc")
        return int(p.value)

    def free(self, p: int):
        self._ok(self._rt.hipFree(C.c_void_p(p)), "hipFree")

    def memset_async(self, p: int, value: int, nbytes: int, s: int):
        self._ok(self._rt.hipMemsetAsync(C.c_void_p(p), value, nbytes, C.c_void_p(s)), "hipMemsetAsync")

    def delay(self, s: int, repeats: int = None, nbytes: int = None):
        """Filler work on stream `s` (never on the null stream: a delay there would order everything).  The scratch buffer is allocated
        by the first delay and kept for the life of the process (one helper per process: `hip()`)."""
        if not s:
            return
        repeats = FILLER_REPEATS if repeats is None else repeats
        nbytes = FILLER_BYTES if nbytes is None else nbytes
        if nbytes > FILLER_BYTES:
            raise ValueError("delay: at most the scratch buffer's FILLER_BYTES per memset")
        if self._scratch is None:
            self._scratch = self.malloc(FILLER_BYTES)
        for k in range(repeats):
            self.memset_async(self._scratch, k & 0xff, nbytes, s)


_hip = None


def hip() -> Hip:
    global _hip
    if _hip is None:
        _hip = Hip()
    return _hip


class Streams:
    """Streams of one test: created on demand, synchronised and destroyed when the block ends (after the contexts, which the test closes
    inside the block)."""

    def __init__(self):
        self.h = hip()
        self._made = []

    def __enter__(self):
        return self

    def new(self, non_blocking: bool = True) -> int:
        s = self.h.stream_create(non_blocking)
        self._made.append(s)
        return s

    def __exit__(self, *exc):
        for s in self._made:
            self.h.stream_synchronize(s)
            self.h.stream_destroy(s)
        self._made = []
        return False
