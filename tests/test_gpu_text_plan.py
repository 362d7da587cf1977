"""The micro-batch plan of the device text route (csrc/textparse.hip text_batch_plan, text_host_lines) through fwgpu_debug_text_plan against the
NumPy restatement below: placement offsets, launch windows and their statistics, the compacted list of host lines -- element for element."""
import ctypes as C

import numpy as np
import pytest

from fwumious_wabbit_amd import capi

pytestmark = pytest.mark.gpu

DEVICE_OK, NEEDS_HOST, HOST_DONE = 1, 2, 3
NONE = 0xFFFFFFFF


def plan_ref(status, n_take, mb, learn_before):
    """status: [nlines, 4] uint32 {status (| flags above the low byte), length, LR entries, FFM entries}"""
    st = status[:, 0] & 0xFF
    counts = (st == DEVICE_OK) | (st == HOST_DONE)
    length = np.where(counts, status[:, 1], 0).astype(np.uint64)
    n_lr = np.where(counts, status[:, 2], 0).astype(np.uint64)
    n_ffm = np.where(counts, status[:, 3], 0).astype(np.uint64)
    rec_off = np.zeros(n_take + 1, dtype=np.uint64)
    rec_off[1:] = np.cumsum(length[:n_take], dtype=np.uint64)
    n_learn = min(learn_before, n_take)
    windows = [(f, min(f + mb, n_learn)) for f in range(0, n_learn, mb)] + [(f, min(f + mb, n_take)) for f in range(n_learn, n_take, mb)]
    stats = np.zeros((len(windows), 7), dtype=np.uint64)
    for w, (f, e) in enumerate(windows):
        stats[w] = [e - f, rec_off[e] - rec_off[f], n_lr[f:e].max(), n_ffm[f:e].max(), length[f:e].max(), n_lr[f:e].sum(), n_ffm[f:e].sum()]
    return rec_off, stats, np.flatnonzero(st == NEEDS_HOST).astype(np.uint32)


def plan_dev(status, n_take, mb, learn_before):
    nlines = len(status)
    status = np.ascontiguousarray(status, dtype=np.uint32)
    dst_off = np.full(max(n_take, 1), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    rec_off = np.full(n_take + 1, 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    n_windows_max = n_take + 2
    stats = np.full((n_windows_max, 7), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    host = np.full(max(nlines, 1), 0xAAAAAAAA, dtype=np.uint32)
    nw, nh = C.c_uint32(12345), C.c_uint32(12345)
    capi.check(capi.lib().fwgpu_debug_text_plan(capi.ptr(status) if nlines else None, nlines, n_take, mb, learn_before, capi.ptr(dst_off), capi.ptr(rec_off),
                                                C.byref(nw), capi.ptr(stats), capi.ptr(host), C.byref(nh), None))
    assert np.all(stats[nw.value:] == 0xAAAAAAAAAAAAAAAA) and np.all(host[nh.value:] == 0xAAAAAAAA)  # nothing written past the counts
    return dst_off[:n_take], rec_off, stats[: nw.value], host[: nh.value]


def make_status(nlines, seed, kind="mixed"):
    rng = np.random.default_rng(seed)
    s = np.zeros((nlines, 4), dtype=np.uint32)
    if kind == "all-host":
        s[:, 0] = NEEDS_HOST
        return s
    s[:, 0] = rng.choice([DEVICE_OK, DEVICE_OK, DEVICE_OK, HOST_DONE], size=nlines)
    s[:, 0] |= rng.choice([0, 1 << 8], size=nlines).astype(np.uint32)  # the record-rule flag rides above the status byte
    if kind == "with-host":
        s[rng.random(nlines) < 0.1, 0] = NEEDS_HOST
    s[:, 1] = rng.integers(9, 200, size=nlines)
    if kind == "long":  # lengths up to 65 535 words: with some 70 000 of them the offsets pass 2^32
        s[:, 1] = rng.integers(60000, 65536, size=nlines)
        s[rng.integers(0, max(nlines, 1), size=min(nlines, 3)), 1] = 65535
    s[:, 2] = rng.integers(1, 5000, size=nlines)
    s[:, 3] = rng.integers(0, 5000, size=nlines)
    s[(s[:, 0] & 0xFF) == NEEDS_HOST, 1:] = 0  # as the status pass leaves such a line
    return s


def check(status, n_take, mb, learn_before):
    want_off, want_stats, want_host = plan_ref(status, n_take, mb, learn_before)
    dst_off, rec_off, stats, host = plan_dev(status, n_take, mb, learn_before)
    assert np.array_equal(rec_off, want_off)
    assert np.array_equal(dst_off, want_off[:n_take])
    assert stats.shape == want_stats.shape and np.array_equal(stats, want_stats)
    assert np.array_equal(host, want_host)
    return want_off, want_stats


def boundaries(n_take, mb):
    """none, 0, the middle of a window, a window edge"""
    out = [NONE, 0]
    if n_take > 1:
        out.append(min(n_take - 1, mb * (n_take // mb // 2) + max(mb // 2, 1)) if mb > 1 else n_take // 2)
    if n_take > mb:
        out.append(mb * max(1, n_take // mb // 2))
    return sorted(set(out))


@pytest.mark.parametrize("nlines", [0, 1, 63, 64, 65, 1024, 1025, 5000])
@pytest.mark.parametrize("mb", [1, 7, 64, 4096])
def test_plan_matches_restatement(nlines, mb):
    status = make_status(nlines, 1000 * mb + nlines, "with-host" if nlines % 2 else "mixed")
    for n_take in sorted({nlines, max(nlines - 1, 0), 0}):
        for lb in boundaries(n_take, mb):
            check(status, n_take, mb, lb)


@pytest.mark.parametrize("nlines", [1, 64, 65, 1025, 5000])
def test_all_needs_host_compacts_to_every_line(nlines):
    status = make_status(nlines, nlines, "all-host")
    off, stats = check(status, nlines, 64, NONE)
    assert not off.any() and np.array_equal(stats[:, 0], [min(64, nlines - f) for f in range(0, nlines, 64)]) and not stats[:, 1:].any()


def test_offsets_pass_2_to_the_32():
    status = make_status(70000, 9, "long")
    for mb, lb in ((4096, NONE), (7, 33333), (64, 64 * 500)):
        off, stats = check(status, 70000, mb, lb)
        assert int(off[-1]) > 1 << 32 and int(stats[:, 4].max()) == 65535


def test_refuses_what_it_cannot_plan():
    status = make_status(8, 3)
    out = np.zeros(64, dtype=np.uint64)
    n = C.c_uint32()
    L = capi.lib()
    host = np.zeros(8, dtype=np.uint32)
    args = (capi.ptr(out), capi.ptr(out), C.byref(n), capi.ptr(out), capi.ptr(host), C.byref(n), None)
    assert L.fwgpu_debug_text_plan(capi.ptr(status), 8, 9, 4, NONE, *args) == capi.ERR_INVALID  # n_take > nlines
    assert L.fwgpu_debug_text_plan(capi.ptr(status), 8, 8, 0, NONE, *args) == capi.ERR_INVALID  # micro_batch 0
