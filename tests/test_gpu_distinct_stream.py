"""The line distinct (sre_hip_distinct_lines) on a caller's gated non-blocking stream, one entry in the shape of
tests/test_gpu_caller_stream.py's table (reference on the null stream, gate closed and asserted closed, result equal), and
in a call order that shares the scanner's tables with the tally and the lookup: d_ttab, d_tslot, d_fval and d_vval."""
import pytest

import sregex_amd as S
from test_gpu_caller_stream import (Src, call_lookup, gated_check, guards_intact, keys, kv, kv_text, kvw_scanner, line_cap,      # noqa: F401
                                    run, tally_call)                                                  # (keys, kv: fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


def distinct_call(which, min_count=1, max_count=0, invert=False):
    def call(sc, src, n, hs, spans):
        L = line_cap(n)
        return run(sc, [n + 16, 8 * L, 8 * L, 32 * L],
                   lambda out, kc, kl, idx: sc.distinct_lines(src, n, out.ptr, out.cap, [1], L, which, min_count, max_count,
                                                              invert=invert, keycount_ptr=kc.ptr, keycount_cap=L, keyline_ptr=kl.ptr,
                                                              keyline_cap=L, index_ptr=idx.ptr, index_cap=L, hip_stream=hs))
    return call


@pytest.mark.parametrize("which", [S.HIP_DISTINCT_FIRST, S.HIP_DISTINCT_LAST, S.HIP_DISTINCT_EVERY], ids=["first", "last", "every"])
def test_the_call_with_its_producer_pending(gpu, keys, kv, which):
    real, decoy = kv
    lo = 2 if which == S.HIP_DISTINCT_EVERY else 1
    with S.Pool() as pool:
        got, sc = gated_check(lambda: kvw_scanner(pool, keys=keys), distinct_call(which, lo), real, decoy)
        assert 40 <= got[0].nkeys <= 60 and 0 < got[0].nselected < got[0].nkeyed
        assert sc.engine == S.ENGINE_SCAN and sc.last_lines_device == 1 and sc.last_line_batches == 1


def test_calls_that_share_the_tables_in_one_order(gpu, keys, kv):
    """tally_lines on a larger buffer with a larger table, then LAST, the lookup, FIRST on one scanner: each equals its
    answer on a fresh scanner"""
    real, _ = kv
    big = Src(kv_text(77, 4.4) + b"\n" + kv_text(78, 4.4) + b"\n" + kv_text(79, 4.4))
    try:
        assert len(big.lines) > 2 * len(real.lines)
        steps = [(tally_call([1, 2]), big), (distinct_call(S.HIP_DISTINCT_LAST), real), (call_lookup, real),
                 (distinct_call(S.HIP_DISTINCT_FIRST, 2, 0, invert=True), real), (tally_call([1]), real),
                 (distinct_call(S.HIP_DISTINCT_LAST, 1, 3), real)]
        with S.Pool() as pool:
            sc = kvw_scanner(pool, keys=keys)
            for k, (call, src) in enumerate(steps):
                got = call(sc, src.ptr, len(src.data), None, src.lines)
                want = call(kvw_scanner(pool, keys=keys), src.ptr, len(src.data), None, src.lines)
                assert got == want and guards_intact(got), ("step", k)
                assert got[0].nselected > 0
    finally:
        big.free()
