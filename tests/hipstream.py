"""A caller's stream with a gate: a non-blocking HIP stream whose pending work is held back while a test makes its call.

A ctypes binding of the HIP runtime the library is linked against (libamdhip64.so, as tools/h2d_sizes.py binds it):
nothing is compiled and torch is not needed.

The mechanism in use is hipLaunchHostFunc.  GatedStream.produce() queues on the stream a host function that blocks until
a threading.Event is set (waiting at most 2 s, so it can never block for good), a device-to-device copy of the real
input over the buffer the call will read, and a HIP event behind that copy; a threading.Timer sets the Event after `hold`
seconds.  The runtime stalls the stream behind the host function with a barrier that only the function's return
releases, so while the gate is closed the GPU is idle and the buffer still holds what it held before: anything the
library issues off the caller's stream runs at once, against those stale bytes, and a call that returns before its work
is complete returns while the copy is still pending.  copy_pending() (hipEventQuery == hipErrorNotReady on the event
behind the copy) lets a test assert, immediately before its call, that the gate is in fact closed: a runtime on which the
host function did not hold the stream would fail that assertion, not pass vacuously.

HOLD is 50 ms.  A test times its null-stream reference call on the warm scanner and asserts that it took less than
hold / 10, so the whole host-side issue of the gated call falls inside the closed gate.  The reference calls measured
0.2 to 2.4 ms on an MI355X but for one kind: scan_lines with find-all counting on the NFA tier (302 lines, a horizon of
256 bytes: many rounds, each read back by the host) took 7.2 ms, so that kind's gate stays closed for FIND_ALL_HOLD,
100 ms, and its guard is a tenth of that; and sre_hip_streams_feed of the table-driven set (24 streams of first-match
Pike with two groups, chunks of up to 3000 bytes), whose three reference feeds took 6.9, 14.8 and 19.5 ms, so its gate
stays closed for TABLE_SET_HOLD, 400 ms (the NFA-tier set's feeds took 0.1 ms and keep HOLD).
"""
import ctypes
import threading
import time

HOLD = 0.05
FIND_ALL_HOLD = 0.1
TABLE_SET_HOLD = 0.4
GATE_TIMEOUT = 2.0

hipSuccess = 0
hipErrorNotReady = 600
hipStreamNonBlocking = 0x01
hipMemcpyDeviceToDevice = 3

_vp, _sz = ctypes.c_void_p, ctypes.c_size_t
HostFn = ctypes.CFUNCTYPE(None, _vp)

_hip = None


def runtime():
    """libamdhip64.so with the entry points used here declared"""
    global _hip
    if _hip is None:
        hip = ctypes.CDLL("libamdhip64.so")
        for name, args in {
            "hipStreamCreateWithFlags": [ctypes.POINTER(_vp), ctypes.c_uint],
            "hipStreamDestroy": [_vp],
            "hipStreamSynchronize": [_vp],
            "hipMemcpyAsync": [_vp, _vp, _sz, ctypes.c_int, _vp],
            "hipLaunchHostFunc": [_vp, HostFn, _vp],
            "hipEventCreate": [ctypes.POINTER(_vp)],
            "hipEventRecord": [_vp, _vp],
            "hipEventQuery": [_vp],
            "hipEventDestroy": [_vp],
        }.items():
            fn = getattr(hip, name)
            fn.restype = ctypes.c_int
            fn.argtypes = args
        _hip = hip
    return _hip


def _ok(rc, what):
    if rc != hipSuccess:
        raise RuntimeError("%s failed: hipError %d" % (what, rc))


class GatedStream:
    """a hipStreamNonBlocking stream; .handle is what a call takes as hip_stream"""

    def __init__(self):
        self.hip = runtime()
        self.handle = _vp()
        _ok(self.hip.hipStreamCreateWithFlags(ctypes.byref(self.handle), hipStreamNonBlocking), "hipStreamCreateWithFlags")
        self.released = threading.Event()       # the gate of the last produce()
        self.timed_out = False                  # a gate that nobody opened within GATE_TIMEOUT
        self.opened_at = None                   # time.perf_counter() when the last gate opened
        self._keep = []                         # the CFUNCTYPE objects, alive as long as the stream
        self._timers = []
        self._events = []
        self._behind = None

    def produce(self, dst_ptr, src_ptr, nbytes, hold=HOLD):
        """queue the gate, then the copy of nbytes from src_ptr over dst_ptr; the gate opens after `hold` seconds.
        Waits for nothing."""
        gate = threading.Event()

        def wait(_user):
            if not gate.wait(GATE_TIMEOUT):
                self.timed_out = True

        def open_gate():
            self.opened_at = time.perf_counter()
            gate.set()

        fn = HostFn(wait)
        self._keep.append(fn)
        self.released, self.opened_at = gate, None
        _ok(self.hip.hipLaunchHostFunc(self.handle, fn, None), "hipLaunchHostFunc")
        try:
            if nbytes:
                _ok(self.hip.hipMemcpyAsync(dst_ptr, src_ptr, nbytes, hipMemcpyDeviceToDevice, self.handle), "hipMemcpyAsync")
            ev = _vp()
            _ok(self.hip.hipEventCreate(ctypes.byref(ev)), "hipEventCreate")
            self._events.append(ev)
            _ok(self.hip.hipEventRecord(ev, self.handle), "hipEventRecord")
            self._behind = ev
            timer = threading.Timer(hold, open_gate)
            timer.start()
        except BaseException:
            open_gate()         # the gate is queued and no timer will open it
            raise
        self._timers.append(timer)      # started timers only: close() joins them

    def copy_pending(self):
        """the copy of the last produce() has not run yet"""
        rc = self.hip.hipEventQuery(self._behind)
        if rc not in (hipSuccess, hipErrorNotReady):
            raise RuntimeError("hipEventQuery failed: hipError %d" % rc)
        return rc == hipErrorNotReady

    def synchronize(self):
        _ok(self.hip.hipStreamSynchronize(self.handle), "hipStreamSynchronize")

    def close(self):
        """open every gate, wait for the stream and destroy it"""
        if not self.handle:
            return
        for t in self._timers:
            t.join()
        try:
            self.synchronize()
        finally:
            for ev in self._events:
                self.hip.hipEventDestroy(ev)
            self.hip.hipStreamDestroy(self.handle)
            self.handle = _vp()
            self._events, self._timers = [], []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def timed(fn):
    """(fn(), host seconds it took)"""
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0
