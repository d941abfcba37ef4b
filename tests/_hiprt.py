"""A minimal ctypes binding of the HIP runtime that libcytohip.so ITSELF loaded, for the tests that hand the library a stream of
their own (tests/test_caller_stream_gpu.py).

A stream means something only to the runtime that made it, and a process can hold more than one copy of the runtime (a PyTorch
wheel bundles its own): so the library is loaded first (_lib.lib()), the libamdhip64 it pulled in is found in /proc/self/maps, and
THAT file is opened again, which yields the copy already mapped.  Do not import torch beside this module.

Only what the stream tests need is bound: streams, hipMemcpyAsync, events.  hipStreamQuery leaves hipErrorNotReady behind as the
thread's last error, and the library checks hipGetLastError() after its launches (CYTO_HIP(hipGetLastError())): stream_ready()
therefore clears it after every such query, as the library's own cache_release does (csrc/core.hip).
"""
import ctypes

from cytospace_amd import _lib

hipSuccess = 0
hipErrorNotReady = 600
hipStreamNonBlocking = 1
hipMemcpyDeviceToDevice = 3

_rt = None


class HipError(RuntimeError):
    pass


def runtime_path():
    """The path of the one libamdhip64 mapped into this process once libcytohip.so is loaded."""
    _lib.lib()
    paths = set()
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split(None, 5)
            if len(parts) == 6 and "libamdhip64" in parts[5]:
                paths.add(parts[5].strip())
    if len(paths) != 1:
        raise HipError(f"expected one HIP runtime in this process, found {sorted(paths)} (was torch imported?)")
    return paths.pop()


def runtime():
    global _rt
    if _rt is None:
        rt = ctypes.CDLL(runtime_path())
        vp, vpp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)
        for name, args in (("hipStreamCreateWithFlags", [vpp, ctypes.c_uint]), ("hipStreamDestroy", [vp]),
                           ("hipStreamSynchronize", [vp]), ("hipStreamQuery", [vp]), ("hipGetLastError", []),
                           ("hipMemcpyAsync", [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]),
                           ("hipEventCreate", [vpp]), ("hipEventRecord", [vp, vp]), ("hipEventSynchronize", [vp]),
                           ("hipEventElapsedTime", [ctypes.POINTER(ctypes.c_float), vp, vp]), ("hipEventDestroy", [vp])):
            fn = getattr(rt, name)
            fn.argtypes, fn.restype = args, ctypes.c_int
        _rt = rt
    return _rt


def _check(code, what):
    if code != hipSuccess:
        runtime().hipGetLastError()
        raise HipError(f"{what} failed with HIP error {code}")


def stream_create():
    """A non-blocking stream (it does not synchronise with the NULL stream); returns its address."""
    s = ctypes.c_void_p()
    _check(runtime().hipStreamCreateWithFlags(ctypes.byref(s), hipStreamNonBlocking), "hipStreamCreateWithFlags")
    return s.value


def stream_destroy(s):
    _check(runtime().hipStreamDestroy(s), "hipStreamDestroy")


def stream_synchronize(s):
    _check(runtime().hipStreamSynchronize(s), "hipStreamSynchronize")


def stream_ready(s):
    """False while work queued on s has not finished.  The not-ready code is taken off the thread's last-error slot again."""
    code = runtime().hipStreamQuery(s)
    if code == hipErrorNotReady:
        runtime().hipGetLastError()
        return False
    _check(code, "hipStreamQuery")
    return True


def memcpy_d2d_async(dst, src, nbytes, s):
    _check(runtime().hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync")


def event_create():
    e = ctypes.c_void_p()
    _check(runtime().hipEventCreate(ctypes.byref(e)), "hipEventCreate")
    return e.value


def event_record(e, s):
    _check(runtime().hipEventRecord(e, s), "hipEventRecord")


def event_synchronize(e):
    _check(runtime().hipEventSynchronize(e), "hipEventSynchronize")


def event_elapsed_ms(e0, e1):
    ms = ctypes.c_float()
    _check(runtime().hipEventElapsedTime(ctypes.byref(ms), e0, e1), "hipEventElapsedTime")
    return float(ms.value)


def event_destroy(e):
    _check(runtime().hipEventDestroy(e), "hipEventDestroy")
