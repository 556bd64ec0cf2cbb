"""The wide NFA tier (sre_nfa_wide.h, sre_hip_nfa_wide.hip): programs whose thread sets need more than 64
bits run on the bit-parallel NFA scanner with 128- or 256-bit sets per lane instead of the one-lane VM.
Results equal the oracle and the reference CLI's lines in every mode."""
import random

import pytest

import sregex_amd as S
import harness

pytestmark = pytest.mark.gpu

WIDE = [([rb"(?:a|b)*a(?:a|b){30}@"], None), ([rb"[ab]*a[ab]{40}c[^x]{40}@"], 128),
        ([rb"[ab]*a[ab]{100}c[^x]{100}@"], 256)]


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def expect(ora, prog, ncaps, data):
    """(first-match record, count record) the batched API must return (as test_gpu_parity)"""
    nov = 2 * (ncaps + 1)
    allm = harness.findall(ora, prog, ncaps, data)
    final = allm[-1][0]
    matches = allm[:-1]
    first = [matches[0][0], 1] + matches[0][1:] if matches else [S.SRE_DECLINED, 0] + [-1] * nov
    if matches:
        cnt = [S.SRE_ERROR if final == S.SRE_ERROR else matches[-1][0], len(matches)] + matches[-1][1:]
    else:
        cnt = [final, 0] + [-1] * nov
    return first, cnt


def listable(prog):
    return sum(1 for line in prog.dump().splitlines()
               if line.split()[1:2] and line.split()[1] in ("char", "in", "notin", "any", "match"))


def subject(rng, k, m, n):
    """random a/b runs with planted matches of [ab]*a[ab]{k}c[^x]{m}@"""
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.choice(b"ab") for _ in range(rng.randrange(k // 2, 2 * k + 2)))
        r = rng.random()
        if r < 0.3:
            out += b"c" + bytes(rng.choice(b"abz ") for _ in range(rng.choice([m - 1, m, m + 3]))) + b"@"
        elif r < 0.5:
            out += b"x@c\n"
    return bytes(out[:n])


def test_engine_nfa_takes_programs_wider_than_64_bits(gpu):
    ora = harness.OracleEngine()
    rng = random.Random(5150)
    for pats, bits in WIDE:
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            assert listable(prog) > 64
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT):
                sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
                assert sc.engine == S.ENGINE_NFA
                print(pats, mode, sc.kernel_name, sc.nfa_bits)
                assert sc.nfa_bits in (64, 128, 256)
                if bits:
                    assert sc.nfa_bits == bits, (pats, sc.nfa_bits)
                    assert sc.kernel_name.startswith("sre_k_nfa_wide<%d," % (bits // 64)), sc.kernel_name
                datas = [subject(rng, 40, 40, n) for n in (0, 100, 3000, 70000)]
                bufs = [S.DeviceBuffer.from_bytes(d) for d in datas]
                got = sc.scan([b.ptr for b in bufs], [len(d) for d in datas])
                for d, g in zip(datas, got):
                    first, cnt = expect(ora, prog, re.ncaps, d)
                    if mode == S.HIP_PIKE_FIRST:
                        assert g == first, (pats, len(d), g, first)
                    elif mode == S.HIP_PIKE_COUNT:
                        assert g == cnt, (pats, len(d), g, cnt)
                    else:
                        assert g[:2] == [0 if first[0] >= 0 else S.SRE_DECLINED, 1 if first[0] >= 0 else 0]
                for b in bufs:
                    b.free()


def test_a_64_bit_form_after_merging_runs_on_the_shift_and_kernel(gpu):
    """66 threads merge into 33 bits: the 64-bit shift-and kernel takes the form, not the wide one"""
    ora = harness.OracleEngine()
    rng = random.Random(31)
    with S.Pool() as pool:
        re = S.parse(pool, [rb"(?:a|b)*a(?:a|b){30}@"])
        prog = S.compile(pool, re)
        datas = [bytes(rng.choice(b"ab@ ") for _ in range(n)) for n in (50, 4000, 30000)]
        bufs = [S.DeviceBuffer.from_bytes(d) for d in datas]
        for mode in (S.HIP_THOMPSON, S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT):
            for engine in (S.ENGINE_AUTO, S.ENGINE_NFA):
                sc = S.Scanner(pool, prog, mode, engine)
                assert sc.engine == S.ENGINE_NFA and sc.nfa_bits == 64
                assert sc.kernel_name == "sre_k_nfa_sa<true, true, true, true, 0, false>", sc.kernel_name
                got = sc.scan([b.ptr for b in bufs], [len(d) for d in datas])
                for d, g in zip(datas, got):
                    first, cnt = expect(ora, prog, re.ncaps, d)
                    if mode == S.HIP_THOMPSON:
                        assert g[:2] == [0 if first[0] >= 0 else S.SRE_DECLINED, 1 if first[0] >= 0 else 0]
                    else:
                        assert g == (first if mode == S.HIP_PIKE_FIRST else cnt), (mode, len(d), g)
        for b in bufs:
            b.free()


def nfa_why(pool, prog, capfd):
    """the builder's reason when ENGINE_NFA declines the program (printed by the library)"""
    capfd.readouterr()
    try:
        S.Scanner(pool, prog, S.HIP_PIKE_FIRST, S.ENGINE_NFA)
    except RuntimeError:
        return capfd.readouterr().err.strip()
    return None


def test_reference_runs_with_more_than_64_threads(gpu, blocks, capfd):
    bad, rows, width = [], [], []
    for blk in blocks:
        subj = bytes.fromhex(blk["s"])
        for name, regexes, flags, multi, ref in harness.block_variants(blk):
            if ref["rc"] != 0:
                continue
            with S.Pool() as pool:
                prog = S.compile(pool, S.parse(pool, regexes, flags, multi))
                nt = listable(prog)
                if nt <= 64:
                    continue
                sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST, S.ENGINE_AUTO)
                if sc.engine == S.ENGINE_SCAN:
                    rows.append((blk["name"], name, nt, "scan"))
                    continue
                if sc.engine != S.ENGINE_NFA:
                    why = nfa_why(pool, prog, capfd)
                    rows.append((blk["name"], name, nt, "vm: %s" % why))
                    # a decline for width must only come from more than 256 bits after merging
                    if why is None or "more than 64" in why or ("256 thread bits" in why and nt <= 256):
                        width.append((blk["name"], name, nt, why))
                    continue
                rows.append((blk["name"], name, nt, sc.kernel_name))
                buf = S.DeviceBuffer.from_bytes(subj)
                rec = sc.scan([buf.ptr], [len(subj)])[0]
                th = S.Scanner(pool, prog, S.HIP_THOMPSON, S.ENGINE_AUTO).scan([buf.ptr], [len(subj)])[0]
                buf.free()
                nov = 2 * (ref["ncaps"] + 1)
                line = ("pike match %d%s" % (rec[0], harness._fmt_caps(rec[2:], nov)) if rec[0] >= 0
                        else "pike no match")
                tl = "thompson " + ("match" if th[0] == 0 else "no match")
                if line != ref["res"][4] or tl != ref["res"][0]:
                    bad.append((blk["name"], name, line, ref["res"][4], tl, ref["res"][0]))
    with capfd.disabled():
        print("admission of the reference runs with more than 64 list-able threads:")
        for r in rows:
            print("  ", *r)
    assert not bad, bad
    assert not width, width
    assert sum(1 for r in rows if r[3].startswith("sre_k_nfa_wide")) >= 3, rows


@pytest.mark.parametrize("seg", [64, 192, 4096])
def test_random_differential_vs_oracle_and_vm(gpu, seg):
    ora = harness.OracleEngine()
    rng = random.Random(777 + seg)
    zoo = [([rb"[ab]*a[ab]{40}c[^x]{40}@"], 40, 40), ([rb"[ab]*a[ab]{100}c[^x]{100}@"], 100, 100),
           ([rb"(?:a|b)*a(?:a|b){45}@"], 45, 0), ([rb"[ab]*a[ab]{50}c[^x]{30}$"], 50, 30),
           ([rb"\b[ab]*a[ab]{60}c[^x]{20}\b"], 60, 20), ([rb"^[ab]*a[ab]{40}c[^x]{40}@"], 40, 40),
           ([rb"[ab]*a[ab]{40}c", rb"x[^y]*y[ab]{70}@"], 40, 40)]
    for pats, k, m in zoo:
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            datas = [subject(rng, k, m, rng.choice([0, 1, 63, 200, 1000, 5000, 20000])) for _ in range(6)]
            bufs = [S.DeviceBuffer.from_bytes(d) for d in datas]
            ptrs, lens = [b.ptr for b in bufs], [len(d) for d in datas]
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_FIRST, S.HIP_PIKE_COUNT):
                try:
                    sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
                except RuntimeError:
                    assert mode == S.HIP_PIKE_COUNT, pats      # look-ahead and ^ programs keep the VM for find-all
                    continue
                sc.set_segment_bytes(seg)
                got = sc.scan(ptrs, lens)
                assert sc.last_fixups <= 6, (pats, seg, mode, sc.last_fixups)
                vm = S.Scanner(pool, prog, mode, S.ENGINE_VM).scan(ptrs, lens)
                for d, g, v in zip(datas, got, vm):
                    assert g == v, (pats, seg, mode, len(d), g, v)
                    first, cnt = expect(ora, prog, re.ncaps, d)
                    want = first if mode == S.HIP_PIKE_FIRST else cnt if mode == S.HIP_PIKE_COUNT else None
                    if want is not None:
                        assert g == want, (pats, seg, mode, len(d), g, want)
            for b in bufs:
                b.free()


LOOKUP_ZOO = [[rb"x.{0,20}y[ab]{60}c"], [rb"x.{0,40}y[ab]{60}c"], [rb"[ab]*a[ab]{60}cx.{0,60}@"],
              [rb"x.{0,100}y[ab]{60}c"], [rb"[ab]*a[ab]{40}c[^x]{40}@"], [rb"(?:a|b)*a(?:a|b){30}@"],
              [rb"\b[ab]*a[ab]{50}cx.{0,20}$"]]


@pytest.mark.parametrize("options", [0, 4, 16, 4 | 8])
def test_lookup_variants_vs_oracle_and_vm(gpu, options, monkeypatch):
    """programs whose forms need several lookups (long optional chains: 3, 5, 9, 13 hot bytes, one of them
    near the LDS budget at 256 bits), and the build options through SRE_HIP_NFA_WIDE: 4 = the plain slices
    (11-16 lookups), 16 = 256-bit sets for everything — every NL variant of the kernel runs on the device"""
    monkeypatch.setenv("SRE_HIP_NFA_WIDE", str(options))
    ora = harness.OracleEngine()
    rng = random.Random(9000 + options)
    kernels = set()
    for pats in LOOKUP_ZOO:
        with S.Pool() as pool:
            re = S.parse(pool, pats)
            prog = S.compile(pool, re)
            datas = [bytes(rng.choice(b"abxyc@ \n") for _ in range(rng.choice([0, 70, 900, 6000]))) for _ in range(5)]
            datas.append(b"x" + b"ab" * 8 + b"y" + b"a" * 60 + b"c@ " + subject(rng, 40, 40, 3000))
            bufs = [S.DeviceBuffer.from_bytes(d) for d in datas]
            ptrs, lens = [b.ptr for b in bufs], [len(d) for d in datas]
            for mode in (S.HIP_THOMPSON, S.HIP_PIKE_FIRST):
                try:
                    sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
                except RuntimeError:
                    continue            # (the option's form does not fit the LDS budget)
                kernels.add(sc.kernel_name)
                sc.set_segment_bytes(192)
                got = sc.scan(ptrs, lens)
                assert sc.last_fixups <= 6, (pats, mode, sc.last_fixups)
                vm = S.Scanner(pool, prog, mode, S.ENGINE_VM).scan(ptrs, lens)
                for d, g, v in zip(datas, got, vm):
                    assert g == v, (pats, options, mode, sc.kernel_name, len(d), g, v)
                    if mode == S.HIP_PIKE_FIRST:
                        first, _ = expect(ora, prog, re.ncaps, d)
                        assert g == first, (pats, options, sc.kernel_name, len(d), g, first)
            for b in bufs:
                b.free()
    print(options, sorted(kernels))
    nls = {int(k.split(",")[1]) for k in kernels if k.startswith("sre_k_nfa_wide")}
    assert len(nls) >= 2, kernels


def test_forms_beyond_the_lds_budget_keep_the_exact_vm(gpu):
    """`x.{0,114}y[ab]{60}c` needs more lookup tables than one workgroup's LDS holds: declined, AUTO keeps the
    exact VM and its answer"""
    ora = harness.OracleEngine()
    data = b"zz x" + b"q" * 100 + b"y" + b"ab" * 30 + b"c tail"
    with S.Pool() as pool:
        re = S.parse(pool, [rb"x.{0,114}y[ab]{60}c"])
        prog = S.compile(pool, re)
        with pytest.raises(RuntimeError):
            S.Scanner(pool, prog, S.HIP_PIKE_FIRST, S.ENGINE_NFA)
        sc = S.Scanner(pool, prog, S.HIP_PIKE_FIRST, S.ENGINE_AUTO)
        assert sc.engine == S.ENGINE_VM
        buf = S.DeviceBuffer.from_bytes(data)
        first, _ = expect(ora, prog, re.ncaps, data)
        assert sc.scan([buf.ptr], [len(data)])[0] == first
        buf.free()


def test_program_that_never_forgets_gets_exact_entry_sets(gpu):
    ora = harness.OracleEngine()
    pats = [rb"x[^y]*y[ab]*a[ab]{40}c[^x]{40}@"]
    body = b"abccc" * ((16 << 20) // 5)
    data = b"x" + body + b"y" + b"a" * 42 + b"c" + b"b" * 40 + b"@ "
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        small = b"x" + b"abccc" * 3000 + data[-90:]
        first_small, _ = expect(ora, prog, re.ncaps, small)
        assert first_small[0] >= 0
        buf = S.DeviceBuffer.from_bytes(data)
        for mode in (S.HIP_PIKE_FIRST, S.HIP_THOMPSON):
            sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
            assert sc.nfa_bits == 128
            rec = sc.scan([buf.ptr], [len(data)])[0]
            shift = len(data) - len(small)
            if mode == S.HIP_PIKE_FIRST:
                # the match runs from the x at 0 to the @ at the end
                assert first_small[:3] == [0, 1, 0] and len(first_small) == 4, first_small
                assert rec == [0, 1, 0, first_small[3] + shift], rec
            else:
                assert rec[:2] == [0, 1], rec
            print(mode, "fixups", sc.last_fixups, "exact passes", sc.last_exact_passes)
            assert sc.last_fixups <= 6, sc.last_fixups
            assert sc.last_exact_passes >= 1
        buf.free()


@pytest.mark.parametrize("pats,bits", [([rb"[ab]*a[ab]{40}c[^x]{40}@"], 128), ([rb"[ab]*a[ab]{100}c[^x]{100}@"], 256)])
def test_large_stream_closed_form(gpu, pats, bits):
    """1 GiB of gen-data ("abccc" x n + tail) with a match in the tail: checked against the oracle on a short stream"""
    ora = harness.OracleEngine()
    k = 40 if bits == 128 else 100
    tail = b" " + b"a" * (k + 1) + b"c" + b"b" * k + b"@ "
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        small = S.gen_data_host(30000, tail)
        first, _ = expect(ora, prog, re.ncaps, small)
        assert first[0] >= 0
        off = [v - len(small) for v in first[2:]]       # the match lies in the tail
        big = 1 << 30
        L = S.gen_data_length(big, len(tail))
        buf = S.DeviceBuffer(big)
        assert gpu.sre_hip_gen_data(buf.ptr, L, tail, len(tail), None) == 0
        for mode in (S.HIP_PIKE_FIRST, S.HIP_THOMPSON):
            sc = S.Scanner(pool, prog, mode, S.ENGINE_AUTO)
            assert sc.engine == S.ENGINE_NFA and sc.nfa_bits == bits
            rec = sc.scan([buf.ptr], [L])[0]
            if mode == S.HIP_PIKE_FIRST:
                assert rec == [first[0], 1] + [v + L for v in off], rec
            else:
                assert rec[:2] == [0, 1], rec
            assert sc.last_fixups == 0
        buf.free()


def test_compat_exec_on_a_whole_buffer_runs_on_the_wide_tier(gpu):
    ora = harness.OracleEngine()
    eng = harness.ProductEngine()
    pats = [rb"[ab]*a[ab]{40}c[^x]{40}@"]
    rng = random.Random(99)
    data = subject(rng, 40, 40, 1 << 20)
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        o = ora.pike(prog, re.ncaps)
        want = o.exec(data, True)
        wov = list(o.ovector)
        o.close()
        before = S.compat_route_counts()
        p = eng.pike(prog, re.ncaps)
        got = p.exec(data, True)
        gov = list(p.ovector)
        after = S.compat_route_counts()
        assert got == want and (got < 0 or gov == wov), (got, want, gov, wov)
        assert after[0] - before[0] >= 1, (before, after)
        assert after[2] == before[2], (before, after)
        eng.recycle()


def test_scan_lines_equals_the_batched_api(gpu):
    rng = random.Random(4)
    pats = [rb"[ab]*a[ab]{40}c[^x]{40}@"]
    lines = [subject(rng, 40, 40, rng.choice([0, 5, 90, 300, 2000])).replace(b"\n", b" ") for _ in range(300)]
    data = b"\n".join(lines)
    with S.Pool() as pool:
        prog = S.compile(pool, S.parse(pool, pats))
        buf = S.DeviceBuffer.from_bytes(data)
        for mode in (S.HIP_PIKE_FIRST, S.HIP_THOMPSON):
            sc = S.Scanner(pool, prog, mode, S.ENGINE_NFA)
            nl, nr, rows = sc.scan_lines(buf.ptr, len(data), all_lines=True, cap=len(lines) + 1)
            assert nl == len(lines) == nr
            starts, at = [], 0
            for ln in lines:
                starts.append(at)
                at += len(ln) + 1
            recs = S.Scanner(pool, prog, mode, S.ENGINE_NFA).scan([buf.ptr + s for s in starts], [len(x) for x in lines])
            for i, (row, rec) in enumerate(zip(rows, recs)):
                assert row[:3] == [i, starts[i], len(lines[i])], (row[:3], i)
                assert row[3:] == rec, (i, row, rec)
        buf.free()
