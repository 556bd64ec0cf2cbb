"""Line mode against the batched API on the same lines (sre_hip_scan_lines vs sre_hip_scan_enqueue/results).

Shapes: a million 96-byte lines without and with a match on every line (the lines of many_small_probe.py) in
FIRST, COUNT and THOMPSON modes; 4 GiB of those 96-byte lines; 1 GiB of 4 KiB lines.  Per shape the two
calls alternate in one run, each timed by the host clock around the synchronous call; the batched API's host
arrays are built outside the timed region (in calls of at most a million streams: its per-stream buffers grow
with the streams of a call).  Both must report the same matching lines.  Prints one JSON document
(--out also writes it to a file).

    python tools/lines_probe.py [--shapes million,4g,1g4k] [--reps 5] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import sregex_amd as S

L = 96
LINES = {"nomatch": (b"GET /index.html user nobody " + b"x" * 96)[:L - 1] + b"\n",
         "match": (b"GET /index.html user a@abc.cc " + b"x" * 96)[:L - 1] + b"\n"}
PATTERN = rb"([a-z]+)@([a-z]+)\.[a-z]+"
BATCH_CALL = 1 << 20        # streams per batched-API call


def fill(lib, nbytes, block):
    """device buffer of nbytes: `block` repeated (len(block) divides nbytes)"""
    buf = S.DeviceBuffer(nbytes)
    for o in range(0, nbytes, len(block)):
        assert lib.sre_hip_upload(buf.ptr + o, block, len(block)) == 0
    return buf


def time_lines(sc, buf, nbytes, cap, out):
    nl, nr = ctypes.c_size_t(), ctypes.c_size_t()
    t0 = time.perf_counter()
    assert sc.lib.sre_hip_scan_lines(sc.h, buf.ptr, nbytes, 0x0A, 0, out, cap, ctypes.byref(nl), ctypes.byref(nr),
                                     None) == 0
    return time.perf_counter() - t0, nl.value, nr.value


def time_batched(sc, calls, out):
    """calls: [(ptr array, len array, n)]; returns (seconds in the calls, reported lines)"""
    rep, dt = 0, 0.0
    for a, b, n in calls:
        pa = a.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p))
        pb = b.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
        po = out.ctypes.data_as(ctypes.POINTER(ctypes.c_ssize_t))
        t0 = time.perf_counter()
        assert sc.lib.sre_hip_scan_enqueue(sc.h, pa, pb, n, None) == 0
        assert sc.lib.sre_hip_scan_results(sc.h, po) == 0
        dt += time.perf_counter() - t0
        rep += int(np.count_nonzero(out[:n * sc.slots:sc.slots] != S.SRE_DECLINED))
    return dt, rep


def read_ceiling(lib, buf, nbytes, reps=3):
    best = 1e9
    for _ in range(reps):
        lib.sre_hip_synchronize(None)
        t0 = time.perf_counter()
        assert lib.sre_hip_read_ceiling(buf.ptr, nbytes, None) == 0
        lib.sre_hip_synchronize(None)
        best = min(best, time.perf_counter() - t0)
    return nbytes / best / 1e9


def run_shape(lib, pool, prog, name, line, nlines, modes, reps, ceiling=False):
    nbytes = len(line) * nlines
    per_block = 1
    while per_block * 2 * len(line) <= (64 << 20) and nlines % (per_block * 2) == 0:
        per_block *= 2
    buf = fill(lib, nbytes, line * per_block)
    # batched API: the same lines, host arrays outside the timed region
    starts = np.arange(nlines, dtype=np.uint64) * np.uint64(len(line))
    ptrs = starts + np.uint64(buf.ptr)
    lens = np.full(nlines, len(line) - 1, dtype=np.uint64)
    calls = [(ptrs[i:i + BATCH_CALL], lens[i:i + BATCH_CALL], min(BATCH_CALL, nlines - i)) for i in range(0, nlines, BATCH_CALL)]
    res = {"shape": name, "lines": nlines, "line_bytes": len(line), "bytes": nbytes, "modes": {}}
    if ceiling:
        res["read_ceiling_GBps"] = read_ceiling(lib, buf, nbytes)
    for mode, mname in modes:
        sc = S.Scanner(pool, prog, mode)
        cap = min(nlines, 1 << 20)
        out_lines = (ctypes.c_ssize_t * (cap * (3 + sc.slots)))()
        out_batch = np.zeros(min(BATCH_CALL, nlines) * sc.slots, dtype=np.int64)
        time_lines(sc, buf, nbytes, cap, out_lines)             # warm-up: code objects, buffers
        time_batched(sc, calls[:1], out_batch)
        tl, tb = [], []
        for _ in range(reps):
            dt, nl, nr = time_lines(sc, buf, nbytes, cap, out_lines)
            tl.append(dt)
            kms, batches, fix = sc.last_kernel_ms, sc.last_line_batches, sc.last_fixups
            dt, rep = time_batched(sc, calls, out_batch)
            tb.append(dt)
            assert nl == nlines and nr == rep, (nl, nr, rep)
        ml, mb = statistics.median(tl), statistics.median(tb)
        res["modes"][mname] = {
            "kernel": sc.kernel_name, "engine": sc.engine_name, "reported": nr,
            "lines_ms": {"median": ml * 1e3, "min": min(tl) * 1e3, "all": [x * 1e3 for x in tl]},
            "batched_ms": {"median": mb * 1e3, "min": min(tb) * 1e3, "all": [x * 1e3 for x in tb]},
            "lines_over_batched": ml / mb, "lines_GBps": nbytes / ml / 1e9, "batched_GBps": nbytes / mb / 1e9,
            "lines_scan_kernels_ms": kms, "line_batches": batches, "fixups": fix,
            "batched_calls": len(calls),
        }
        print(json.dumps({name: {mname: res["modes"][mname]}}), flush=True)
    buf.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="million,4g,1g4k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = S.load_library()
    assert lib.sre_hip_device_count() >= 1, "no HIP device"
    shapes = args.shapes.split(",")
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    doc = {"tool": "tools/lines_probe.py", "commit": commit, "reps": args.reps, "pattern": PATTERN.decode(),
           "timing": "host clock around each synchronous call; median of reps, line mode and batched API alternating",
           "results": []}
    all_modes = ((S.HIP_PIKE_FIRST, "first"), (S.HIP_PIKE_COUNT, "count"), (S.HIP_THOMPSON, "thompson"))
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        if "million" in shapes:
            for kind, line in LINES.items():
                doc["results"].append(run_shape(lib, pool, prog, "1M x 96 B " + kind, line, 1 << 20, all_modes, args.reps))
        if "4g" in shapes:
            doc["results"].append(run_shape(lib, pool, prog, "4 GiB x 96 B nomatch", LINES["nomatch"], (4 << 30) // 96 >> 19 << 19,
                                            all_modes[:1], max(2, args.reps // 2), ceiling=True))
        if "1g4k" in shapes:
            line = (b"GET /index.html user a@abc.cc " + b"y" * 4096)[:4095] + b"\n"
            doc["results"].append(run_shape(lib, pool, prog, "1 GiB x 4 KiB match", line, 1 << 18, all_modes[:1], args.reps))
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
