"""The scan kernel with more workgroups than the device has CUs: several scan waves share every SIMD, which is where
their issue priority (SRE_SCAN_PRIO, sre_hip_scan.hip) decides who runs.  Priority must change no result.  The form
tests' subjects fit one workgroup; here one 24 MiB stream at the small 256-byte geometry fills the chip one and a half
times over.  One program each of the 2-bit and 4-bit forms, ENGINE_SCAN forced, FIRST, COUNT and Thompson against the
oracle; the form is asserted by name.  The test holds as it stands for a library built with -DSRE_SCAN_PRIO=1, 2 or 3."""
import subprocess
import sys

import pytest

import sregex_amd as S
import harness
from test_gpu_parity import _expect
from test_gpu_scan_forms import MODES, URI, compare

pytestmark = pytest.mark.gpu

SEG = 256                           # segment bytes: 98 305 segments, 385 workgroups of 256 lanes
N = 24 * (1 << 20) + 37             # a ragged last segment
OFFSET = 3                          # the stream starts this far past its buffer's aligned start
FILLER = b"ab cd. x9 "              # bytes of several classes in both programs, no event
# (regexes, event, class bits, FIRST / Thompson form, COUNT form)
PROGRAMS = [
    ([rb"[a-z]+@[a-z]+\.[a-z]+"], b" a@b.c ", 2, "sre_k_scan<1, 2, true, false>", "sre_k_scan<2, 2, true, true>"),
    ([URI], b" abc://abc.cc/ab/c?a=b ", 4, "sre_k_scan<1, 4, false, false>", "sre_k_scan<2, 4, false, true>"),
]


def subject(event):
    """Filler with three events: one that ends inside the warm-up line (the 128 bytes in front) of a segment deep in
    the launch, one in the last 64-byte round of a later segment, one in the stream's last bytes."""
    data = bytearray((FILLER * (N // len(FILLER) + 1))[:N])
    k1, k2 = 70001, 90002           # segments of workgroups 273 and 351: both past the first CU-count workgroups
    for end in (k1 * SEG - 20, (k2 + 1) * SEG - 9, N - 2):
        data[end - len(event):end] = event
    return bytes(data)


@pytest.fixture(scope="module")
def gpu(lib):
    assert lib.sre_hip_device_count() >= 1, "no HIP device: the product has no CPU path"
    return lib


@pytest.fixture(scope="module")
def cus():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked once in a process of its own: torch brings its
    own HIP runtime, which finds no device in a process where the library's runtime already holds it (as it does
    here whenever another GPU test ran first)."""
    out = subprocess.run([sys.executable, "-c",
                          "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         stdout=subprocess.PIPE, timeout=120, check=True)
    return int(out.stdout.decode().split()[-1])


@pytest.mark.parametrize("pats,event,bits,first_form,count_form", PROGRAMS, ids=["2bit", "4bit"])
def test_more_workgroups_than_cus_vs_oracle(gpu, cus, pats, event, bits, first_form, count_form):
    data = subject(event)
    with S.Pool() as pool:
        re = S.parse(pool, pats)
        prog = S.compile(pool, re)
        first, cnt = _expect(harness.OracleEngine(), prog, re.ncaps, data)
        assert first[1] == 1 and cnt[1] == 3, (first, cnt)
        buf = S.DeviceBuffer.from_bytes(b"#" * OFFSET + data)
        try:
            for mode in MODES:
                sc = S.Scanner(pool, prog, mode, S.ENGINE_SCAN)
                want = count_form if mode == S.HIP_PIKE_COUNT else first_form
                assert sc.class_bits == bits and sc.kernel_name == want, (pats, mode, sc.class_bits, sc.kernel_name)
                sc.set_segment_bytes(SEG)
                got = sc.scan([buf.ptr + OFFSET], [len(data)])
                seg = sc.last_segment_bytes
                groups = -(-(-(-len(data) // seg)) // 256)
                assert seg == SEG and groups > cus, (seg, groups, cus)
                compare(got, mode, 0, first, cnt, (pats, seg, groups))
        finally:
            buf.free()
