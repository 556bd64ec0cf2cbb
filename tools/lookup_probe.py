"""The line lookup against the calls a user has without it (sre_hip_lookup_lines vs sre_hip_filter_lines,
sre_hip_tally_lines and extract + download + a Python set).

A million 96-byte log lines, each with k=KEY (five letters) and a mark m=1 / m=0, the program k=([a-z]+) in mode FIRST on
the table-driven scanner, group [1].  A set holds the keys 0 .. S - 1 for S = 1, 4096 and 2^20; of the lines roughly
1 %, 50 % or all carry a key of the set (line i: key i % S) and the mark m=1, the others a key outside it (S + i) and m=0.
Per set size and share
  (a) the whole lookup_lines call (lines and key ids; no index),
  (b) filter_lines with a scanner for m=1, which selects the same lines with no set at all,
  (c) tally_lines of the same group on the same buffer (rows, counts and key ids; max_keys = lines), and
  (d) the host alternative: extract_lines of the group, a download of the rows and a Python set
alternate in one process, each timed by the host clock around the synchronous call: the median of --reps calls after a
warm-up.  keyset_create is timed per size the same way.  Then (e): one run of every configuration under rocprofv3
--kernel-trace --stats in a child process that makes calls (a) and (c); its kernel statistics go to --stats-out, and the
lookup's and the tally's own kernels and the select passes are listed per configuration with their median time per
dispatch.  Prints one JSON document (--out also writes it to a file).

    python tools/lookup_probe.py [--reps 5] [--out FILE] [--stats-out FILE] [--no-profile]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sregex_amd as S
from filter_probe import ms
from extract_probe import stats_top

NLINES = 1 << 20
L = 96
WIDTH = 5                                   # letters of a key: 26^5 > 2 * NLINES
SET_SIZES = (1, 4096, NLINES)
SHARES = (1, 50, 100)                       # per cent of the lines whose key is in the set
PATTERN = rb"k=([a-z]+)"
MARK = rb"m=1"
GROUPS = [1]
HEAD = b"GET /index.html k="
KERNELS = ("sre_k_keyset_probe", "sre_k_tally_insert", "sre_k_tally_keep", "sre_k_extract_select", "sre_k_filter_select")


def key_columns(v):
    return [ord("a") + (v // 26 ** (WIDTH - 1 - j)) % 26 for j in range(WIDTH)]


def is_member(share):
    return (np.arange(NLINES, dtype=np.int64) * 7919) % 100 < share


def upload(lib, raw):
    buf = S.DeviceBuffer(len(raw))
    step = 32 << 20
    for o in range(0, len(raw), step):
        piece = raw[o:o + step]
        assert lib.sre_hip_upload(buf.ptr + o, piece, len(piece)) == 0
    return buf, len(raw)


def fill_lines(lib, size, share):
    """the buffer: line i = HEAD, its key, the mark, a tail of x, a newline; returns (buffer, bytes, member lines)"""
    row = np.frombuffer((HEAD + b"a" * WIDTH + b" m=0 user nobody " + b"x" * L)[:L - 1] + b"\n", dtype=np.uint8)
    a = np.tile(row, (NLINES, 1))
    i = np.arange(NLINES, dtype=np.int64)
    member = is_member(share)
    v = np.where(member, i % size, size + i)
    for j, col in enumerate(key_columns(v)):
        a[:, len(HEAD) + j] = col
    a[:, len(HEAD) + WIDTH + 3] = np.where(member, ord("1"), ord("0"))
    buf, nbytes = upload(lib, a.tobytes())
    return buf, nbytes, int(member.sum())


def fill_set(lib, size):
    """the dictionary: the keys 0 .. size - 1, one a row"""
    a = np.full((size, WIDTH + 1), ord("\n"), dtype=np.uint8)
    for j, col in enumerate(key_columns(np.arange(size, dtype=np.int64))):
        a[:, j] = col
    return upload(lib, a.tobytes())


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def host_alternative(lib, sc, buf, nbytes, out, members):
    """extract the group, bring the rows to the host, test each against a Python set; returns the lines found"""
    info = sc.extract_lines(buf.ptr, nbytes, GROUPS, out.ptr, nbytes)
    rows = out.to_bytes(info.out_bytes).split(b"\n")
    return sum(1 for r in rows if r in members)


def run_set(lib, pool, prog, mark, size, reps):
    dbuf, dbytes = fill_set(lib, size)
    tc = []
    for rep in range(reps + 1):
        dt, ks = timed(lambda: S.KeySet(dbuf.ptr, dbytes, 1))
        assert (ks.rows, ks.distinct) == (size, size)
        if rep:
            tc.append(dt)
        if rep < reps:
            ks.close()
    members = {bytes(key_columns(v)) for v in range(size)}
    out_rows = []
    for share in SHARES:
        buf, nbytes, nmem = fill_lines(lib, size, share)
        out, keyid, counts = S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(8 * NLINES)
        sc, fsc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST), S.Scanner(pool, mark, S.HIP_PIKE_FIRST)
        assert sc.engine == S.ENGINE_SCAN
        tl, tf, tt, th = [], [], [], []
        for rep in range(reps + 1):         # (the first round warms up: code objects, buffers)
            dl, info = timed(lambda: sc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr,
                                                     keyid_cap=NLINES))
            assert sc.last_lines_device == 1
            assert info == S.LookupInfo(NLINES, NLINES, nmem, nmem, nmem * L, nmem, nmem * L), info
            df, finfo = timed(lambda: fsc.filter_lines(buf.ptr, nbytes, out.ptr, nbytes))
            assert finfo == S.FilterInfo(NLINES, nmem, nmem * L, nmem, nmem * L), finfo
            dt, tinfo = timed(lambda: sc.tally_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, NLINES, counts_ptr=counts.ptr,
                                                     counts_cap=NLINES, keyid_ptr=keyid.ptr, keyid_cap=NLINES))
            dh, found = timed(lambda: host_alternative(lib, sc, buf, nbytes, out, members))
            assert found == nmem
            if rep:
                tl.append(dl)
                tf.append(df)
                tt.append(dt)
                th.append(dh)
        out_rows.append({"set_keys": size, "set_slots": ks.slots, "set_device_bytes": ks.device_bytes, "member_share_pct": share,
                         "lines": NLINES, "bytes": nbytes, "members": nmem, "tally_keys": tinfo.nkeys, "kernel": sc.kernel_name,
                         "filter_engine": fsc.engine_name,
                         "keyset_create_ms": ms(tc), "lookup_ms": ms(tl), "filter_ms": ms(tf), "tally_ms": ms(tt),
                         "host_extract_download_set_ms": ms(th),
                         "lookup_over_filter": statistics.median(tl) / statistics.median(tf),
                         "lookup_minus_filter_ms": (statistics.median(tl) - statistics.median(tf)) * 1e3})
        for b in (buf, out, keyid, counts):
            b.free()
    ks.close()
    dbuf.free()
    return out_rows


def child(calls):
    """the run to put under the profiler: `calls` lookup and tally calls per configuration after one warm-up call each"""
    lib = S.load_library()
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST)
        for size in SET_SIZES:
            dbuf, dbytes = fill_set(lib, size)
            ks = S.KeySet(dbuf.ptr, dbytes, 1)
            for share in SHARES:
                buf, nbytes, _ = fill_lines(lib, size, share)
                out, keyid, counts = S.DeviceBuffer(nbytes), S.DeviceBuffer(8 * NLINES), S.DeviceBuffer(8 * NLINES)
                for _ in range(calls + 1):
                    sc.lookup_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, ks, keyid_ptr=keyid.ptr, keyid_cap=NLINES)
                    sc.tally_lines(buf.ptr, nbytes, out.ptr, nbytes, GROUPS, NLINES, counts_ptr=counts.ptr, counts_cap=NLINES,
                                   keyid_ptr=keyid.ptr, keyid_cap=NLINES)
                for b in (buf, out, keyid, counts):
                    b.free()
            ks.close()
            dbuf.free()


def profile(calls, stats_out):
    """(e): the child under rocprofv3; every listed kernel's dispatches in order, per configuration"""
    tmp = tempfile.mkdtemp(prefix="lookup_probe_")
    configs = [(size, share) for size in SET_SIZES for share in SHARES]
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child", "--child-calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=500)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        assert stats and trace, os.listdir(tmp)
        if stats_out:
            shutil.copyfile(stats[0], stats_out)
        with open(trace[0], newline="") as f:
            all_rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        per = []
        for name in KERNELS:
            ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in all_rows if name in r["Kernel_Name"]]
            each = len(ns) // len(configs)
            assert each * len(configs) == len(ns) and each % (calls + 1) == 0, (name, len(ns))
            d = each // (calls + 1)             # dispatches of a round: the lookup call's, then the tally call's
            for i, (size, share) in enumerate(configs):
                mine = ns[i * each + d:(i + 1) * each]
                row = {"kernel": name, "set_keys": size, "member_share_pct": share, "dispatches_per_round": d}
                if name == "sre_k_extract_select":
                    assert d % 2 == 0, d            # per batch: the lookup's pass over the key group; then the tally's
                    row["lookup_median_us"] = statistics.median(x for j, x in enumerate(mine) if j % d < d // 2) / 1e3
                    row["tally_median_us"] = statistics.median(x for j, x in enumerate(mine) if j % d >= d // 2) / 1e3
                else:
                    row["median_us"] = statistics.median(mine) / 1e3
                per.append(row)
        once = {}
        for name in ("sre_k_keyset_fields", "sre_k_keyset_insert"):
            ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in all_rows if name in r["Kernel_Name"]]
            assert len(ns) == len(SET_SIZES), (name, len(ns))
            once[name] = {str(size): x / 1e3 for size, x in zip(SET_SIZES, ns)}
        with open(stats[0], newline="") as f:
            top = stats_top(csv.DictReader(f), 20)
        return per, once, top
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-out", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-calls", type=int, default=5, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child_calls)
        return
    lib = S.load_library()
    assert lib.sre_hip_device_count() >= 1, "no HIP device"
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = None
    doc = {"tool": "tools/lookup_probe.py", "commit": commit, "reps": args.reps, "lines": NLINES, "line_bytes": L,
           "timing": "host clock around each synchronous call; median of reps after a warm-up; lookup_lines (lines and key ids), "
                     "filter_lines of a scanner for the mark that selects the same lines, tally_lines of the same group (rows, "
                     "counts, key ids; max_keys = lines) and extract_lines + download + Python set alternating in one process",
           "pattern": PATTERN.decode(), "mark": MARK.decode(), "groups": GROUPS, "results": []}
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, [PATTERN]))
        mark = S.compile(pool, S.parse(pool, [MARK]))
        for size in SET_SIZES:
            for r in run_set(lib, pool, prog, mark, size, args.reps):
                print(json.dumps(r), flush=True)
                doc["results"].append(r)
    if not args.no_profile:
        per, once, top = profile(3, args.stats_out)
        doc["kernels"] = {"run": "lookup_lines and tally_lines alternating on the same lines under rocprofv3 --kernel-trace --stats, "
                                 "3 calls of each per configuration after a warm-up call; per kernel the dispatches of the warm-up "
                                 "round are left out; the key set's two kernels run once per set size (us)",
                          "kernel_stats_top": top, "keyset_create_us": once, "rows": per}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
