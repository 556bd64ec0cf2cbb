"""Line mode against the batched API on the same lines (sre_hip_scan_lines vs sre_hip_scan_enqueue/results).

Shapes: a million 96-byte lines without and with a match on every line (the lines of many_small_probe.py) in
FIRST, COUNT and THOMPSON modes; 4 GiB of those 96-byte lines; 1 GiB of 4 KiB lines.  Per shape the two
calls alternate in one run, each timed by the host clock around the synchronous call; the batched API's host
arrays are built outside the timed region (in calls of at most a million streams: its per-stream buffers grow
with the streams of a call).  Both must report the same matching lines.  Prints one JSON document
(--out also writes it to a file).

    python tools/lines_probe.py [--shapes million,4g,1g4k] [--reps 5] [--out FILE]

--engine nfa: the same on the bit-parallel NFA tier (scanners created with ENGINE_NFA), FIRST and THOMPSON: the
million-line shapes with a counted-repeat pattern and an IP-address pattern over synthetic log lines, three columns
alternating — line mode on the device, line mode on the per-line host route (SRE_HIP_LINES_NFA_HOST=1) and the
batched API; then the crossover between the short-line kernel (SRE_HIP_LINES_SHORT_MAX = the line length) and the
set pass (SRE_HIP_LINES_SHORT_MAX=0) at line lengths 64 .. 4096 over the same number of bytes.

    python tools/lines_probe.py --engine nfa [--shapes million,ip,crossover] [--reps 5] [--out FILE]
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


# ---- the NFA tier (--engine nfa)

NFA_PATTERN = rb"(?:a|b)*a(?:a|b){7}@"
NFA_LINES = {"nomatch": (b"GET /index.html user nobody " + b"x" * 96)[:L - 1] + b"\n",
             "match": (b"GET /index.html user abaabaabab@abc.cc " + b"x" * 96)[:L - 1] + b"\n"}
IP_PATTERN = rb"\d{1,3}(\.\d{1,3}){3}"
CROSSOVER_LENGTHS = [64, 96, 128, 256, 512, 1024, 2048, 4096]
CROSSOVER_BYTES = 96 << 20


def log_block(nlines, with_ip):
    """synthetic log lines of 50 .. 140 bytes; with_ip: every fourth line holds an address"""
    rng = np.random.default_rng(7)
    out = []
    for i in range(nlines):
        words = [b"Oct 17 12:%02d:%02d host sshd[%d]:" % (i % 60, (7 * i) % 60, 1000 + i % 9000)]
        if with_ip and i % 4 == 0:
            words.append(b"Accepted publickey for user%d from %d.%d.%d.%d port %d" % ((i % 50,) + tuple(int(x) for x in rng.integers(1, 255, 4))
                                                                                    + (int(rng.integers(1024, 65535)),)))
        else:
            words.append(b"session " + (b"opened" if i % 2 else b"closed") + b" for user u" + b"x" * int(rng.integers(0, 60)))
        out.append(b" ".join(words) + b"\n")
    return out


def fill_repeat(lib, nbytes, block):
    """device buffer of nbytes: `block` repeated, the last copy cut at the end of the buffer"""
    buf = S.DeviceBuffer(nbytes)
    chunk = block * max(1, (32 << 20) // len(block))
    for o in range(0, nbytes, len(chunk)):
        piece = chunk[:min(len(chunk), nbytes - o)]
        assert lib.sre_hip_upload(buf.ptr + o, piece, len(piece)) == 0
    return buf


def set_env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def run_nfa_shape(lib, pool, prog, name, block_lines, repeat, modes, reps):
    """block_lines (each ends in a newline) repeated `repeat` times; device route, host route and batched API"""
    block = b"".join(block_lines)
    nlines, nbytes = len(block_lines) * repeat, len(block) * repeat
    buf = fill_repeat(lib, nbytes, block)
    blens = np.array([len(x) for x in block_lines], dtype=np.uint64)
    bstarts = np.concatenate(([0], np.cumsum(blens)[:-1])).astype(np.uint64)
    starts = (np.arange(repeat, dtype=np.uint64)[:, None] * np.uint64(len(block)) + bstarts[None, :]).reshape(-1)
    ptrs = starts + np.uint64(buf.ptr)
    lens = np.tile(blens - np.uint64(1), repeat)
    calls = [(ptrs[i:i + BATCH_CALL], lens[i:i + BATCH_CALL], min(BATCH_CALL, nlines - i)) for i in range(0, nlines, BATCH_CALL)]
    res = {"shape": name, "lines": nlines, "bytes": nbytes, "mean_line_bytes": nbytes / nlines, "modes": {}}
    for mode, mname in modes:
        sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
        cap = min(nlines, 1 << 20)
        out_lines = (ctypes.c_ssize_t * (cap * (3 + sc.slots)))()
        out_batch = np.zeros(min(BATCH_CALL, nlines) * sc.slots, dtype=np.int64)
        t = {"device": [], "host": [], "batched": []}
        info = {}
        for rep in range(reps + 1):     # (the first round warms up: code objects, buffers)
            set_env("SRE_HIP_LINES_NFA_HOST", None)
            dt, nl, nr = time_lines(sc, buf, nbytes, cap, out_lines)
            assert sc.last_lines_device == 1
            info = {"short_lines": sc.last_short_lines, "line_batches": sc.last_line_batches, "fixups": sc.last_fixups,
                    "device_kernels_ms": sc.last_kernel_ms}
            set_env("SRE_HIP_LINES_NFA_HOST", "1")
            dh, nl2, nr2 = time_lines(sc, buf, nbytes, cap, out_lines)
            assert sc.last_lines_device == 0
            set_env("SRE_HIP_LINES_NFA_HOST", None)
            db, nrb = time_batched(sc, calls, out_batch)
            assert nl == nl2 == nlines and nr == nr2 == nrb, (nl, nl2, nr, nr2, nrb)
            if rep:
                t["device"].append(dt)
                t["host"].append(dh)
                t["batched"].append(db)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = {"kernel": sc.kernel_name, "reported": nr}
        row.update(info)
        for k, v in t.items():
            row[k + "_ms"] = {"median": med[k] * 1e3, "min": min(v) * 1e3, "all": [x * 1e3 for x in v]}
        row["host_over_device"] = med["host"] / med["device"]
        row["batched_over_device"] = med["batched"] / med["device"]
        row["device_GBps"] = nbytes / med["device"] / 1e9
        res["modes"][mname] = row
        print(json.dumps({name: {mname: row}}), flush=True)
    buf.free()
    return res


def run_crossover(lib, pool, prog, modes, reps):
    """the short-line kernel against the set pass, every line of one length, the same bytes at every length"""
    rows = []
    rng = np.random.default_rng(11)
    for n in CROSSOVER_LENGTHS:
        nlines = CROSSOVER_BYTES // n
        # 64 distinct lines of a / b (the counted repeat keeps threads alive), one in 64 with a match at its end
        block = []
        for i in range(64):
            body = bytes(97 + int(x) for x in rng.integers(0, 2, n - 1))
            if i == 17:
                body = body[:n - 11] + b"aabaabaab@"
            block.append(body + b"\n")
        block = b"".join(block)
        buf = fill_repeat(lib, nlines * n, block)
        for mode, mname in modes:
            sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
            t = {"short": [], "set_pass": []}
            info = {}
            for rep in range(reps + 1):
                for route, lmax in (("short", str(n)), ("set_pass", "0")):
                    set_env("SRE_HIP_LINES_SHORT_MAX", lmax)
                    dt, nl, nr = time_lines(sc, buf, nlines * n, 0, None)
                    assert nl == nlines and nr == nlines // 64 and sc.last_lines_device == 1
                    assert sc.last_short_lines == (nlines if route == "short" else 0)
                    info[route + "_kernels_ms"] = sc.last_kernel_ms
                    if route == "set_pass":
                        info["segment_bytes"] = sc.last_segment_bytes
                    if rep:
                        t[route].append(dt)
            set_env("SRE_HIP_LINES_SHORT_MAX", None)
            row = {"line_bytes": n, "lines": nlines, "mode": mname, "kernel": sc.kernel_name,
                   "short_ms": statistics.median(t["short"]) * 1e3, "set_pass_ms": statistics.median(t["set_pass"]) * 1e3}
            row["set_pass_over_short"] = row["set_pass_ms"] / row["short_ms"]
            row.update(info)
            rows.append(row)
            print(json.dumps({"crossover": row}), flush=True)
        buf.free()
    return rows


def main_nfa(args, lib, doc):
    shapes = args.shapes.split(",") if args.shapes != "million,4g,1g4k" else ["million", "ip", "crossover"]
    modes = ((S.HIP_PIKE_FIRST, "first"), (S.HIP_THOMPSON, "thompson"))
    doc["engine"] = "nfa"
    doc["timing"] = ("host clock around each synchronous call; median of reps; line mode on the device, line mode on the host "
                     "route (SRE_HIP_LINES_NFA_HOST=1) and the batched API alternating")
    doc["patterns"] = {"counted": NFA_PATTERN.decode(), "ip": IP_PATTERN.decode()}
    del doc["pattern"]
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [NFA_PATTERN]))
        if "million" in shapes:
            for kind, line in NFA_LINES.items():
                doc["results"].append(run_nfa_shape(lib, pool, prog, "1M x 96 B " + kind, [line], 1 << 20, modes, args.reps))
        if "ip" in shapes:
            ipprog = S.compile(pool, S.parse(pool, [IP_PATTERN]))
            for kind in (False, True):
                doc["results"].append(run_nfa_shape(lib, pool, ipprog, "1M log lines, ip " + ("in every fourth" if kind else "in none"),
                                                    log_block(4096, kind), 256, modes, args.reps))
        if "crossover" in shapes:
            doc["crossover"] = {"bytes": CROSSOVER_BYTES, "pattern": NFA_PATTERN.decode(),
                                "columns": "short: SRE_HIP_LINES_SHORT_MAX = the line length (every line through the short-line "
                                           "kernel); set_pass: SRE_HIP_LINES_SHORT_MAX=0 (every line through the set pass)",
                                "rows": run_crossover(lib, pool, prog, modes, args.reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", default="scan", choices=["scan", "nfa"])
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
    if args.engine == "nfa":
        main_nfa(args, lib, doc)
        text = json.dumps(doc, indent=1)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
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
