"""Rates of the wide NFA tier (sre_hip_nfa_wide.hip): kernel and whole-step GB/s over 1 GiB of gen-data for
programs of 64 (after merging), about 100 and about 200 bits, first match and Thompson, against an ENGINE_VM
scanner on 64 KiB of the same input.  Writes profiles/nfa_wide_rate.json."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sregex_amd as S

PEAK = 8000.0          # GB/s, MI355X HBM
CASES = [rb"(?:a|b)*a(?:a|b){30}@", rb"[ab]*a[ab]{45}c[^x]{45}@", rb"[ab]*a[ab]{95}c[^x]{95}@"]


def rate(sc, ptr, n, reps):
    best_k, best_w = 1e30, 1e30
    sc.scan([ptr], [n])                         # warm-up
    for _ in range(reps):
        t0 = time.perf_counter()
        rec = sc.scan([ptr], [n])[0]
        best_w = min(best_w, time.perf_counter() - t0)
        best_k = min(best_k, sc.last_kernel_ms / 1e3)
    return n / best_k / 1e9, n / best_w / 1e9, rec


def main():
    lib = S.load_library()
    big = 1 << 30
    tail = b"aaabbccb"
    L = S.gen_data_length(big, len(tail))
    buf = S.DeviceBuffer(big)
    assert lib.sre_hip_gen_data(buf.ptr, L, tail, len(tail), None) == 0
    small = 64 << 10
    out = {"stream_bytes": L, "vm_bytes": small, "peak_gbs": PEAK, "cases": []}
    for pat in CASES:
        with S.Pool() as pool:
            prog = S.compile(pool, S.parse(pool, [pat]))
            for mode, name in ((S.HIP_PIKE_FIRST, "first"), (S.HIP_THOMPSON, "thompson")):
                sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
                k, w, rec = rate(sc, buf.ptr, L, 3)
                vm = S.Scanner(pool, prog, mode, S.ENGINE_VM)
                t0 = time.perf_counter()
                vrec = vm.scan([buf.ptr], [small])[0]
                vdt = time.perf_counter() - t0
                row = {"pattern": pat.decode(), "mode": name, "kernel": sc.kernel_name, "nfa_bits": sc.nfa_bits,
                       "kernel_gbs": round(k, 1), "kernel_frac": round(k / PEAK, 4), "step_gbs": round(w, 1),
                       "vm_gbs": round(small / vdt / 1e9, 5), "vs_vm": round(w / (small / vdt / 1e9), 1),
                       "fixups": sc.last_fixups, "record": rec[:4], "vm_record_64k": vrec[:4]}
                print(json.dumps(row), flush=True)
                out["cases"].append(row)
    buf.free()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "nfa_wide_rate.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
