"""The reader of a byte-diff stream on the device (csrc/patch_apply.hip) and what stands on it: fwgpu_debug_diff_decode, Image.apply_diff and
the hot patch of a packed regressor.  Streams come from the host codec (P.diff_bytes) on pairs (a, b); the entries the kernels must find are
np.flatnonzero(a != b) + base_offset with b's bytes there, a bad stream's error is the host reader's (P.apply_diff_bytes): all by equality."""
import numpy as np
import pytest

from fwumious_wabbit_amd import capi
from fwumious_wabbit_amd import persistence as P
import publish_cases as K
# the two publishes and the packed comparison are the existing publish tests' own: that file stays as it is, so they are imported, not moved
from test_gpu_publish_diff import _same_packed, two_publishes  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu
T = None


@pytest.fixture(scope="module", autouse=True)
def tile():
    global T
    T = P.debug_decode_geometry()
    assert T >= 64 and T % 16 == 0
    return T


def _check(a, b, base=0, end=None, size=None):
    """the kernels' entries for the host codec's stream of (a, b), twice"""
    stream = P.diff_bytes(a.tobytes(), b.tobytes(), base)
    assert size is None or len(stream) == size
    end = base + a.size if end is None else end
    at = np.flatnonzero(a != b)
    index, to = P.debug_diff_decode(stream, end)
    assert np.array_equal(index, at.astype(np.uint64) + np.uint64(base)) and np.array_equal(to, b[at])
    again = P.debug_diff_decode(stream, end)
    assert np.array_equal(again[0], index) and np.array_equal(again[1], to)
    return stream


def _pair(n, positions, lo=0, hi=256, seed=3):
    """a and b of n bytes that differ at `positions`, b's bytes there in [lo, hi) and a's outside it or different"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=n, dtype=np.uint8)
    b = a.copy()
    v = rng.integers(lo, hi, size=len(positions)).astype(np.uint8)
    b[positions] = v
    a[positions] = np.where(a[positions] == v, v ^ 0x80, a[positions])
    return a, b


@pytest.mark.parametrize("size", ["0", "T-1", "T", "T+1", "3T+5"])
def test_streams_that_end_on_a_tile_edge(size):
    size = {"0": 0, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[size]
    # every byte differs: two stream bytes each, three for the first behind base_offset 12345
    base, n = (12345, (size - 1) // 2) if size % 2 else (0, size // 2)
    for name, a, b in K.patterns(n, T):
        _check(a, b, base, size={"all": size, "none": 0}.get(name))


def test_a_to_byte_first_in_its_tile_and_a_varint_across_an_edge():
    m, r = (T - 4) // 2, (T - 2) // 2
    pos = np.concatenate([np.arange(m), m - 1 + 200 + np.arange(2 + r), [m + 200 + r + 20000]])
    a, b = _pair(int(pos[-1]) + 9, pos)
    stream = _check(a, b, size=2 * T + 3)
    d = np.diff(pos, prepend=0)
    ends = np.cumsum(2 + (d >= 128) + (d >= 16384)) - 1  # every `to` byte's offset in the stream
    assert T in ends and 2 * T + 2 in ends and 2 * T - 2 in ends and len(stream) == ends[-1] + 1


@pytest.mark.parametrize("base", [0, 200], ids=["as-is", "behind-a-two-byte-varint"])
def test_no_top_bit_over_three_tiles_in_both_parities(base):
    pos = np.cumsum(np.random.default_rng(1).integers(1, 128, size=2 * T))
    a, b = _pair(int(pos[-1]) + 1, pos, hi=128)
    stream = np.frombuffer(_check(a, b, base), np.uint8)
    assert stream.size >= 4 * T and (stream[2:] < 128).all() and (stream[0] >= 128) == (base > 0)


def test_to_bytes_of_128_and_more():
    pos = np.cumsum(np.random.default_rng(2).integers(1, 300, size=T))
    _check(*_pair(int(pos[-1]) + 1, pos, lo=128))


def test_a_ten_byte_varint():
    stream = _check(np.zeros(1, np.uint8), np.ones(1, np.uint8), base=2**63 + 5, end=2**64 - 1)
    assert len(stream) == 11


def test_long_gap():
    _check(*K.long_gap(T))


def test_a_stream_that_goes_up_in_three_pinned_chunks():
    a = np.random.default_rng(9).integers(0, 256, size=9 << 20, dtype=np.uint8)
    _check(a, a ^ np.uint8(0x5A), size=18 << 20)  # (8 MiB a chunk: the third waits for the first buffer's transfer)


def _good(n):
    """n entries of two bytes at the indices 0 .. n - 1"""
    return bytes([0, 0x11]) + bytes([1, 0x11]) * (n - 1)


FAULTS = {
    "inside-a-varint": lambda n: bytes([0x85]),
    "before-to": lambda n: bytes([0x05]),
    "eleven-byte-varint": lambda n: bytes([0x81] * 10 + [0x01, 0x11]),
    "ten-byte-varint-ending-in-2": lambda n: bytes([0x80] * 9 + [0x02, 0x11]),
    "zero-delta": lambda n: bytes([0x00, 0x11]),
    "at-the-end": lambda n: P.diff_bytes(b"\0", b"\1", base_offset=1001),  # index n - 1 + 1001 = end
}


def _refused_as_by_the_host(stream, end):
    with pytest.raises(capi.FwgpuError) as want:
        P.apply_diff_bytes(bytes(end), stream)
    with pytest.raises(capi.FwgpuError) as got:
        P.debug_diff_decode(stream, end)
    assert got.value.code == want.value.code == capi.ERR_FORMAT
    assert got.value.message.split(": ", 1)[1] == want.value.message.split(": ", 1)[1]


@pytest.mark.parametrize("in_tile", [0, 2])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_bad_streams_fail_as_the_host_reader_does(fault, in_tile):
    n = 5 + in_tile * T // 2
    rest = b"" if fault in ("inside-a-varint", "before-to") else _good(7)[2:]  # (a stream is truncated at its end only)
    _refused_as_by_the_host(_good(n) + FAULTS[fault](n) + rest, end=n + 1000)


def test_a_zero_delta_in_the_first_entry_is_accepted_and_the_first_of_two_faults_is_reported():
    index, to = P.debug_diff_decode(_good(3), 3)
    assert index.tolist() == [0, 1, 2] and to.tolist() == [0x11] * 3
    _refused_as_by_the_host(_good(5) + FAULTS["zero-delta"](0) + _good(T + 9)[2:] + FAULTS["eleven-byte-varint"](0), end=3 * T)
    _refused_as_by_the_host(_good(5) + FAULTS["ten-byte-varint-ending-in-2"](0) + _good(T + 9)[2:] + FAULTS["zero-delta"](0), end=3 * T)


def test_image_apply_diff(two_publishes):
    t = two_publishes
    img0, img1 = P.Image.load(t["f0"]), P.Image.load(t["f1"])
    with pytest.raises(capi.FwgpuError) as e:
        img0.apply_diff(t["stream"][:-1])
    assert e.value.code == capi.ERR_FORMAT and "ends inside an entry" in e.value.message and img0.read() == t["bytes0"]
    assert img0.apply_diff(b"") == 0 and img0.read() == t["bytes0"]
    assert img0.apply_diff(t["stream"]) == t["changed"]
    assert img0.read() == t["bytes1"] and img0.diff(img1) == b""
    mutated = bytearray(t["bytes0"])
    for i in (3, t["header_bytes"] - 1, t["header_bytes"], len(mutated) - 1):  # two header bytes, the section's first and last
        mutated[i] ^= 0x41
    assert img0.apply_diff(P.diff_bytes(t["bytes1"], bytes(mutated))) >= 4
    assert img0.read() == bytes(mutated)
    img0.close()
    img1.close()


def test_hot_patch_over_several_decode_tiles(tmp_path):
    vw = K.vwmap()
    mi, re = K.model(n=300)
    f0, f1 = str(tmp_path / "a.fw"), str(tmp_path / "b.fw")
    P.save_inference_regressor(f0, mi, vw, re, quantize_weights=True)
    re.table_write(capi.TABLE_FFM_W, [5.0], offset=1001)  # a new maximum: the increment moves and with it nearly every bucket
    P.save_inference_regressor(f1, mi, vw, re, quantize_weights=True)
    stream, changed = P.diff_bytes(open(f0, "rb").read(), open(f1, "rb").read(), with_changed=True)
    assert len(stream) > 3 * T
    recs, off = K.records(200, first=1000)
    mi_p, _, r0 = P.new_regressor_from_filename(f0, immutable=True, packed=True)
    _, _, r1 = P.new_regressor_from_filename(f1, immutable=True, packed=True)
    assert r0.apply_diff(stream) == changed
    _same_packed(r0, r1, mi_p, recs, off)
    for x in (re, r0, r1):
        x.close()
