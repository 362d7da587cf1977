"""Weight tables for the quantiser tests (test_gpu_quantize.py, test_quantize_cpu.py): a seeded normal table at FFM scale and crafted tables that
put the quantiser's every rounding decision and the kernels' every edge (first / last element, the tail of a length that is no multiple of 4) to
work.  The crafted tables use no random generator: their bytes are the same everywhere, so the host quantiser's output on them is committed.

Each crafted case is (name, table, check) where check(buckets u16[n], increment, min) asserts on the HOST quantiser's output that the table
produces the bucket pattern it was made for (the special values sit at fixed small indices, so the checks need n >= MIN_CHECKED_LEN)."""
import numpy as np

MIN_CHECKED_LEN = 63
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099)
# the kernels' grid is capped at 2048 workgroups of 256 lanes, four weights per lane (csrc/fwgpu_internal.h kQuantGridCap): one sweep of the
# grid covers 2^21 weights, this length makes it wrap
WRAP_LENGTH = (1 << 21) + 4099


def normal_table(n, seed=5):
    return (np.random.default_rng(seed).standard_normal(n) * 0.08).astype(np.float32)


def _filler(n, lo, hi, seed):
    """n deterministic values strictly inside (lo, hi)"""
    u = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed * 7919 + 12345)) >> np.uint64(5)) & np.uint64(0xFFFFFF)
    return (lo + (hi - lo) * (0.05 + 0.9 * u.astype(np.float64) / float(1 << 24))).astype(np.float32)


def _put(a, pairs):
    for i, v in pairs:
        if i < len(a):
            a[i] = v
    return a


def _f16(x):
    return int(np.array([x], dtype=np.float32).astype(np.float16).view(np.uint16)[0])


def split(blob, n):
    """(increment, min, buckets u16[n]) of a quantised block"""
    hdr = np.frombuffer(blob[:8], dtype="<f4")
    return np.float32(hdr[0]), np.float32(hdr[1]), np.frombuffer(blob[8:8 + 2 * n], dtype="<u2")


def crafted(n):
    cases = []

    def extremes(name, i_min, i_max, seed):
        a = _filler(n, -0.25, 0.35, seed)
        a[i_max] = 0.4
        a[i_min] = -0.3

        def check(q, inc, mn):
            assert mn == np.float32(-0.3) and q[i_min] == 0
            assert inc == np.float32((np.float32(0.4) - np.float32(-0.3)) / np.float32(65025.0))
            assert q[i_max] == _f16(65025) == 0x7bf0
        cases.append((name, a, check))

    tail = list(range(n - max(n % 4, 1), n))  # the elements past the last whole group of four (the last element when there is none)
    extremes("min-first", 0, n // 2, 1)
    extremes("max-first", n // 2, 0, 2)
    extremes("min-last", n - 1, n // 3, 3)
    extremes("max-last", n // 3, n - 1, 4)
    extremes("min-in-tail", tail[0], n // 2 if len(tail) == 1 else tail[-1], 5)
    extremes("max-in-tail", n // 2 if len(tail) == 1 else tail[-1], tail[0], 6)

    # header {increment 1, min 0}: the quotient IS the weight
    halves = [0.5, 1.5, 2.5, 3.5, 100.5, 1000.5, 2046.5]
    a = _put(_filler(n, 0.0, 65025.0, 7), [(0, 0.0), (1, 65025.0)] + [(2 + j, v) for j, v in enumerate(halves)])

    def check_halves(q, inc, mn):
        assert inc == 1.0 and mn == 0.0
        for j, v in enumerate(halves):  # half away from zero: 2.5 -> 3, where round-half-even would say 2
            assert q[2 + j] == _f16(np.floor(v) + 1), (v, q[2 + j])
    cases.append(("quotients-on-half", a, check_halves))

    # bucket numbers above 2048, where f16 steps by 2, 4, ... 32: exact ties go to the even mantissa
    ties = [(2049.0, 2048), (2051.0, 2052), (4098.0, 4096), (4102.0, 4104), (4097.5, 4096), (32784.0, 32768), (32816.0, 32832), (2049.4, 2048),
            (2050.5, 2052), (40000.3, 40000), (65000.0, 64992)]
    a = _put(_filler(n, 0.0, 65025.0, 8), [(0, 0.0), (1, 65025.0)] + [(2 + j, v) for j, (v, _) in enumerate(ties)])

    def check_ties(q, inc, mn):
        assert inc == 1.0 and mn == 0.0
        for j, (v, want) in enumerate(ties):
            assert q[2 + j] == _f16(want) and float(np.array([q[2 + j]], dtype=np.uint16).view(np.float16)[0]) == want, (v, want, q[2 + j])
    cases.append(("f16-ties", a, check_ties))

    # the minimum rounds UP to 0.1: the weights below it get negative bucket numbers
    a = _put(_filler(n, 0.11, 0.49, 9), [(0, 0.09996), (1, 0.5), (2, 0.09999)])

    def check_negative(q, inc, mn):
        assert mn == np.float32(0.1)
        assert q[0] & 0x8000 and q[0] & 0x7fff and q[2] & 0x8000 and q[2] & 0x7fff
        assert np.array([q[0]], dtype=np.uint16).view(np.float16)[0] == -7.0
    cases.append(("negative-buckets", a, check_negative))

    # [0, 0.00014]: the maximum rounds DOWN to 0.0001 and the top weights land past 65504: infinity
    a = _put(_filler(n, 0.0, 0.00014, 10), [(0, 0.0), (1, 0.00014), (2, 0.00012)])

    def check_overflow(q, inc, mn):
        assert mn == 0.0 and inc == np.float32(np.float32(0.0001) / np.float32(65025.0))
        assert q[1] == 0x7c00 and q[2] == 0x7c00 and q[0] == 0
        assert (q == 0x7c00).sum() >= 2 and (q < 0x7c00).sum() >= 1
    cases.append(("overflow-to-infinity", a, check_overflow))

    # denormal weights inside the range, and as the minimum
    den = np.array([1e-40, -1e-41, 1.4e-45, -1.4e-45], dtype=np.float32)
    assert (den != 0).all() and (np.abs(den) < np.finfo(np.float32).tiny).all()
    a = _put(_filler(n, -0.3, 0.3, 11), [(0, -0.3), (1, 0.3), (2, 0.0)] + [(3 + j, v) for j, v in enumerate(den)])

    def check_denormal(q, inc, mn):
        assert mn == np.float32(-0.3)
        for j in range(len(den)):
            assert q[3 + j] == q[2]  # (the bucket of zero)
    cases.append(("denormal-weights", a, check_denormal))
    a = _put(_filler(n, 0.01, 0.49, 12), [(0, den[0]), (1, 0.5)])

    def check_denormal_min(q, inc, mn):
        assert mn == 0.0 and not np.signbit(mn) and q[0] == 0 and q[1] == _f16(65025)
    cases.append(("denormal-minimum", a, check_denormal_min))

    # a -0.0 that is no extreme
    a = _put(_filler(n, -0.2, 0.3, 13), [(0, -0.2), (1, 0.3), (2, -0.0), (3, 0.0)])

    def check_neg_zero(q, inc, mn):
        assert np.signbit(a[2]) and not np.signbit(a[3]) and q[2] == q[3] and 0 < q[2] < 0x7c00
    cases.append(("negative-zero-inside", a, check_neg_zero))
    return cases


def host_route_tables(n=257):
    """tables the contract sends to the host quantiser: (name, table)"""
    base = _filler(n, -0.3, 0.3, 21)
    nan = base.copy()
    nan[n // 2] = np.nan
    inf = base.copy()
    inf[n - 2] = np.inf
    return [("constant", np.full(n, 0.125, dtype=np.float32)), ("one-nan", nan), ("plus-inf", inf),
            ("max-rounds-onto-min", _filler(n, 0.10001, 0.10004, 22))]


def takes_device_route(blob, table):
    """what the contract says about this table, from the host quantiser's header"""
    inc = np.frombuffer(blob[:4], dtype="<f4")[0]
    return bool(np.isfinite(table).all() and np.isfinite(inc) and inc != 0)
