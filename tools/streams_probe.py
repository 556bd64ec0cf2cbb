"""Stream sets (sre_hip_streams_feed) beside two yardsticks on the same device buffers.

For {1, 64, 1024, 16384} streams x {16 KiB, 256 KiB, 1 MiB, 16 MiB} chunks (cells above --max-bytes
per call are left out), the headline program and BASELINE configs[2]'s 12 regexes, gen-data
streams generated on the device: aggregate GB/s of
  set_first   one feed of a fresh set (every stream's first chunk, no eof),
  set_next    the feed behind it (every stream carries its state in; streams the first chunk
              closed are ignored by it — `open_after_first` says how many were left),
  batch       sre_hip_scan_batch over the same chunks as whole streams (the ceiling: same
              bytes, nothing carried),
  compat      the compat API fed ONE stream in chunks of that size from host memory
              (what tools/stream_probe.py measures), once per chunk size.
Median of --reps after a warm-up, the set and the batched API alternating; host clock around the
synchronous calls.  Prints one JSON document (--out also writes it).

    python tools/streams_probe.py [--reps 5] [--max-bytes N] [--out FILE]
    python tools/streams_probe.py --one 1024x1048576      # that cell of the headline program only
                                                          # (the run to put under rocprofv3)
    python tools/streams_probe.py --engine nfa [--out profiles/streams_nfa_rate.json]
        the same shapes on the NFA tier (StreamSet(..., engine=ENGINE_NFA), Thompson): three programs the
        step automaton declines, at 64, 64 and 128 bits; the yardstick is sre_hip_scan_batch with
        SRE_HIP_ENGINE_NFA on the same chunks (no compat column: chunks of such programs go to the exact VM)
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

import sregex_amd as S

PROGRAMS = {
    "headline": [rb"[a-z]+@[a-z]+\.[a-z]+"],
    "configs2_12_regexes": [b"a", b"ab", b"c", b"a(bc)", b"e(f)", b"gh", b"A", b"b", b"BLAH", rb"\s+", b"abcd", b"bc"],
}
NFA_PROGRAMS = {
    "nfa_a7": [rb"(?:a|b)*a(?:a|b){7}@"],
    "nfa_a20c30": [rb"(?:a|b)*a[ab]{20}c[^x]{30}@"],
    "nfa_wide_a45c45": [rb"[ab]*a[ab]{45}c[^x]{45}@"],
}
STREAMS = [1, 64, 1024, 16384]
CHUNKS = [16 << 10, 256 << 10, 1 << 20, 16 << 20]


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def compat_rate(pool, prog, ncaps, chunk):
    """one stream of max(8 chunks, 64 MiB) through sre_vm_pike_exec from host memory; second pass"""
    total = max(8 * chunk, 64 << 20)
    data = S.gen_data_host(total, b" a@abc.cc ")
    buf = ctypes.create_string_buffer(data, len(data))
    rate = None
    for _ in range(2):
        with S.Pool() as ep:
            ctx = S.PikeCtx(ep, prog, ncaps)
            t0 = time.perf_counter()
            off, rc, fed = 0, S.SRE_AGAIN, 0
            while rc == S.SRE_AGAIN and off < len(data):
                k = min(chunk, len(data) - off)
                rc = ctx.exec(None, off + k >= len(data), want_pending=False, base=buf, offset=off, length=k)
                off += k
                fed += k
            rate = fed / (time.perf_counter() - t0) / 1e9
    return rate


def run_cell(lib, pool, prog, big, n, chunk, reps, yardstick=True, nfa=False):
    ptrs = (ctypes.c_void_p * n)(*[big.ptr + i * chunk for i in range(n)])
    lens = (ctypes.c_size_t * n)(*([chunk] * n))
    eofs = (ctypes.c_ubyte * n)(*([0] * n))
    if nfa:
        ss = S.StreamSet(pool, prog, S.HIP_THOMPSON, n, engine=S.ENGINE_NFA)
        sc = S.Scanner(pool, prog, S.HIP_THOMPSON, S.ENGINE_NFA)
    else:
        ss = S.StreamSet(pool, prog, S.HIP_PIKE_FIRST, n)
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
    out_b = (ctypes.c_ssize_t * (n * sc.slots))()
    everyone = list(range(n))
    t_first, t_next, t_batch = [], [], []
    open_after = launches = fixups = None
    for rep in range(reps + 1):
        ss.reset(everyone)
        a = clock(lambda: ss.feed_raw(ptrs, lens, eofs))
        out = ss._out
        open_after = sum(1 for i in range(n) if out[i * ss.slots + 1] == S.StreamSet.OPEN)
        b = clock(lambda: ss.feed_raw(ptrs, lens, eofs))
        launches, fixups = ss.last_launches, ss.last_fixups
        c = None
        if yardstick:
            c = clock(lambda: lib.sre_hip_scan_batch(sc.h, ptrs, lens, n, out_b, None))
        if rep:                 # the first round is the warm-up
            t_first.append(a)
            t_next.append(b)
            if c is not None:
                t_batch.append(c)
    nbytes = n * chunk
    med = lambda t: statistics.median(t)
    row = {"streams": n, "chunk": chunk, "bytes_per_call": nbytes,
           "set_first_GBps": nbytes / med(t_first) / 1e9, "set_first_us": med(t_first) * 1e6,
           "set_next_GBps": nbytes / med(t_next) / 1e9, "set_next_us": med(t_next) * 1e6,
           "open_after_first": open_after, "launches_per_call": launches, "fixups": fixups,
           "context_bytes": ss.device_bytes}
    if t_batch:
        row["batch_GBps"] = nbytes / med(t_batch) / 1e9
        row["batch_us"] = med(t_batch) * 1e6
        row["set_first_over_batch"] = med(t_first) / med(t_batch)
        row["set_next_over_batch"] = med(t_next) / med(t_batch)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-bytes", type=int, default=16 << 30)
    ap.add_argument("--one", default=None, help="STREAMSxCHUNK: that cell of the headline program only, no yardsticks")
    ap.add_argument("--out", default=None)
    ap.add_argument("--engine", default="scan", choices=["scan", "nfa"], help="nfa: the NFA tier's programs and yardstick")
    args = ap.parse_args()
    nfa = args.engine == "nfa"
    lib = S.load_library()
    assert lib.sre_hip_device_count() >= 1, "no HIP device"
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    doc = {"tool": "tools/streams_probe.py", "commit": commit, "reps": args.reps,
           "timing": "host clock around each synchronous call; median of reps after a warm-up round; set and batched API alternating",
           "kernels": (["sre_k_streams_nfa_prologue", "sre_k_nfa / sre_k_nfa_sa / sre_k_nfa_wide", "sre_k_nfa_verify_a/b/c",
                        "sre_k_streams_nfa_tail"] if nfa else
                       ["sre_k_streams_prologue", "sre_k_scan<1, BITS>", "sre_k_verify_a/b/b2/c", "sre_k_streams_tail"]),
           "results": {}}
    cells = [(n, c) for n in STREAMS for c in CHUNKS if n * c <= args.max_bytes]
    if args.one:
        n, c = (int(x) for x in args.one.split("x"))
        cells = [(n, c)]
    biggest = max(n * c for n, c in cells)
    big = S.DeviceBuffer(biggest)
    assert lib.sre_hip_gen_data(big.ptr, biggest, b"", 0, None) == 0
    assert lib.sre_hip_synchronize(None) == 0
    for name, pats in (NFA_PROGRAMS if nfa else PROGRAMS).items():
        if args.one and name not in ("headline", "nfa_a7"):
            continue
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            sc = S.Scanner(pool, prog, S.HIP_THOMPSON, S.ENGINE_NFA) if nfa else S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
            res = {"scan_kernel": sc.kernel_name, "cells": [], "compat_GBps": {}}
            if nfa:
                res["nfa_bits"] = sc.nfa_bits
            if not args.one and not nfa:
                for c in CHUNKS:
                    res["compat_GBps"][str(c)] = compat_rate(pool, prog, re.ncaps, c)
                    print(json.dumps({name: {"compat_chunk": c, "GBps": res["compat_GBps"][str(c)]}}), flush=True)
            for n, c in cells:
                row = run_cell(lib, pool, prog, big, n, c, args.reps, yardstick=not args.one, nfa=nfa)
                if str(c) in res["compat_GBps"]:
                    row["set_first_over_compat_rate"] = row["set_first_GBps"] / res["compat_GBps"][str(c)]
                res["cells"].append(row)
                print(json.dumps({name: row}), flush=True)
            doc["results"][name] = res
    big.free()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
