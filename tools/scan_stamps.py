#!/usr/bin/env python3
"""When and where every workgroup of the scan kernel ran: one stamped launch of bench.py's headline shape and of its 128 x
64 MiB shape, from a library built with -DSRE_SCAN_STAMPS=1 (sre_hip_scan.hip) given through SREGEX_AMD_LIB as for
tools/ab_bench.py.  Each shape runs in a child process under its own time limit.

usage: SREGEX_AMD_LIB=PATH/libsregex.so scan_stamps.py --label NAME [--out profiles/scan_prio_stamps.json] [--timeout 240]
The result goes under "NAME" into the --out file (other labels in it are kept), per shape:
  end_spread      end times of the workgroups relative to the kernel's start, as shares of the kernel time
  drain           slot time between a workgroup's end and the kernel's end / (slots x kernel time); `unused_slots` of the
                  slots never held a workgroup and are counted in `drain_with_unused`
  by_age          per start rank on its CU (0 = oldest): mean duration, mean end, over all CUs
  key_functions   share of the CUs whose co-resident workgroups (overlapping in time) get distinct values of f(blockIdx.x)
A record is lane 0's: its workgroup's first wave.  Times are wall_clock64() ticks of 10 ns.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TICK_NS = 10.0


class Stamp(ctypes.Structure):
    _fields_ = [("block", ctypes.c_uint32), ("grid", ctypes.c_uint32), ("hw_id", ctypes.c_uint32), ("xcc_id", ctypes.c_uint32),
                ("t_entry", ctypes.c_uint64), ("t_tables", ctypes.c_uint64), ("t_end", ctypes.c_uint64)]


def where(s):
    """(XCC, SE, SH, CU) from the HW_ID and XCC_ID registers: CU_ID [11:8], SH_ID [12], SE_ID [15:13]; XCC_ID [3:0]"""
    return (s.xcc_id & 15, (s.hw_id >> 13) & 7, (s.hw_id >> 12) & 1, (s.hw_id >> 8) & 15)


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def analyse(recs, cus, per_cu, kernel_ms):
    t0 = min(r.t_entry for r in recs)
    t1 = max(r.t_end for r in recs)
    T = float(t1 - t0)
    ends = [(r.t_end - t0) / T for r in recs]
    by_cu = {}
    for r in recs:
        by_cu.setdefault(where(r), []).append(r)
    slots = cus * per_cu
    drain = sum(t1 - r.t_end for r in recs)
    # slots that never held a workgroup: what the launch leaves of cus x per_cu when it is one round
    unused = max(0, slots - len(recs))
    ages = {}
    for rs in by_cu.values():
        rs.sort(key=lambda r: r.t_entry)
        for k, r in enumerate(rs):
            ages.setdefault(k, []).append(r)
    by_age = []
    for k in sorted(ages):
        rs = ages[k]
        by_age.append({"rank": k, "workgroups": len(rs),
                       "mean_start": statistics.mean((r.t_entry - t0) / T for r in rs),
                       "mean_duration": statistics.mean((r.t_end - r.t_entry) / T for r in rs),
                       "mean_walk": statistics.mean((r.t_end - r.t_tables) / T for r in rs),
                       "mean_end": statistics.mean((r.t_end - t0) / T for r in rs),
                       "max_end": max((r.t_end - t0) / T for r in rs)})
    funcs = {"b // %d" % cus: lambda b: b // cus, "b % 4": lambda b: b % 4, "(b // 8) % 4": lambda b: (b // 8) % 4,
             "(b // 32) % 4": lambda b: (b // 32) % 4, "(b // 64) % 4": lambda b: (b // 64) % 4,
             "(b // %d) %% 4" % (cus // 8): lambda b: (b // (cus // 8)) % 4}
    keys = {}
    for name, f in funcs.items():
        ok = n = 0
        for rs in by_cu.values():
            # co-resident: the workgroups of the CU that overlap its first one's end
            first_end = min(r.t_end for r in rs)
            co = [r for r in rs if r.t_entry < first_end]
            if len(co) < 2:
                continue
            n += 1
            ok += len({f(r.block) for r in co}) == len(co)
        keys[name] = ok / n if n else None
    return {"workgroups": len(recs), "cus_seen": len(by_cu), "slots": slots, "unused_slots": unused,
            "kernel_ticks": int(T), "kernel_ms_from_ticks": T * TICK_NS * 1e-6, "kernel_ms_event": kernel_ms,
            "per_cu_counts": {str(k): sum(1 for rs in by_cu.values() if len(rs) == k) for k in sorted({len(rs) for rs in by_cu.values()})},
            "table_copy_mean": statistics.mean((r.t_tables - r.t_entry) / T for r in recs),
            "end_spread": {"min": min(ends), "p10": pct(ends, 0.10), "median": pct(ends, 0.50), "p90": pct(ends, 0.90), "max": 1.0},
            "drain": drain / (len(recs) * T), "drain_with_unused": (drain + unused * T) / (slots * T),
            "by_age": by_age, "key_functions": keys}


def child(shape):
    import torch
    import sregex_amd as S
    import bench
    torch.cuda.set_device(0)            # (as bench.py: torch's HIP runtime first, the library shares it)
    lib = S.load_library()
    if not hasattr(lib, "sre_hip_debug_scan_stamps"):
        raise SystemExit("the library was not built with -DSRE_SCAN_STAMPS=1")
    lib.sre_hip_debug_scan_stamps.restype = ctypes.c_int
    lib.sre_hip_debug_scan_stamps.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    assert lib.sre_hip_set_device(0) == 0
    hstream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    many = shape == "many"
    spec = bench.workload_spec("many" if many else "cfg2", S, (8 if many else 4) * bench.GIB)
    res = bench.Resident(torch, lib, hstream)
    ptrs = res.fill(spec["lens"], spec["tails"], spec.get("block", 0), spec.get("body"))
    torch.cuda.synchronize()
    cap = 1 << 16
    buf = torch.zeros(cap * ctypes.sizeof(Stamp), dtype=torch.uint8, device="cuda")
    pool = S.Pool()
    prog = S.compile(pool, S.parse(pool, spec["pats"]))
    sc = S.Scanner(pool, prog, spec["mode"], spec.get("engine", S.ENGINE_AUTO))
    for _ in range(3):
        spec["check"](sc.scan(ptrs, spec["lens"], hstream))
    assert lib.sre_hip_debug_scan_stamps(buf.data_ptr(), cap) == 0
    recs = sc.scan(ptrs, spec["lens"], hstream)
    kernel_ms, kernel, fixups = sc.last_kernel_ms, sc.kernel_name, sc.last_fixups
    assert lib.sre_hip_debug_scan_stamps(None, 0) == 0
    spec["check"](recs)
    raw = bytes(buf.cpu().numpy())
    stamps = (Stamp * cap).from_buffer_copy(raw)
    # records are in start order over every launch of the call: the first launch's are the first `grid` of them
    grid = stamps[0].grid
    first = [stamps[i] for i in range(min(grid, cap))]
    assert grid > 0 and all(r.grid == grid and r.t_end >= r.t_tables >= r.t_entry > 0 for r in first), "incomplete records"
    assert len({r.block for r in first}) == grid
    later = sum(1 for i in range(grid, cap) if stamps[i].grid != 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = analyse(first, cus, 3 if spec["mode"] == S.HIP_PIKE_COUNT else 4, kernel_ms)
    out.update({"kernel": kernel, "segment_bytes": sc.last_segment_bytes, "fixup_rounds": fixups, "records_of_later_launches": later})
    pool.destroy()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_prio_stamps.json"))
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--child", choices=["headline", "many"])
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if not args.label:
        raise SystemExit("--label NAME")
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    entry, status = {"library": os.environ.get("SREGEX_AMD_LIB", "")}, 0
    for shape in ("headline", "many"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape], cwd=ROOT, stdout=subprocess.PIPE,
                               timeout=args.timeout)
            status = p.returncode
        except subprocess.TimeoutExpired:
            status = 124
        if status != 0:
            print("%s: status %d, stopping" % (shape, status), file=sys.stderr)
            break
        entry[shape] = json.loads(p.stdout.decode().strip().splitlines()[-1])
        e = entry[shape]
        print("%s %s: %d workgroups on %d CUs, kernel %.3f ms, ends %.3f .. 1, drain %.3f (%.3f with unused slots)"
              % (args.label, shape, e["workgroups"], e["cus_seen"], e["kernel_ms_from_ticks"], e["end_spread"]["min"], e["drain"],
                 e["drain_with_unused"]), flush=True)
    doc[args.label] = entry
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
