"""The rule the device decoder's entry boundaries rest on (csrc/patch_apply.hip): byte i of a diff stream is a `to` byte exactly when the run
of top-bit-clear bytes that ends at i - 1 has odd length, the run reaching back to the last top-bit-set byte or to the stream's start."""
import numpy as np

from fwumious_wabbit_amd import persistence as P


def _varint(v):
    out = []
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    return out + [v]


def test_to_bytes_follow_clear_runs_of_odd_length():
    rng = np.random.default_rng(7)
    for _ in range(300):
        n = int(rng.integers(1, 13))
        # varints of 1 to 9 bytes; twelve deltas below 2^60 sum below 2^64.  One stream in ten is a single entry with a 10-byte varint
        deltas = [int(rng.integers(1, 2 ** int(rng.integers(1, 61)), dtype=np.uint64)) for _ in range(n)]
        if rng.random() < 0.1:
            deltas = [int(rng.integers(2**63, 2**64 - 1, dtype=np.uint64, endpoint=True))]
        to = rng.integers(0, 256, size=len(deltas), dtype=np.uint8)
        pieces = [_varint(d) + [int(t)] for d, t in zip(deltas, to)]
        stream = bytes(b for piece in pieces for b in piece)
        s = np.frombuffer(stream, np.uint8)
        run = np.zeros(s.size + 1, dtype=np.int64)  # run[i]: the length of the clear run that ends at byte i - 1
        for i in range(s.size):
            run[i + 1] = run[i] + 1 if s[i] < 128 else 0
        at = np.flatnonzero(run[:-1] % 2 == 1)
        assert np.array_equal(at, np.cumsum([len(piece) for piece in pieces]) - 1) and np.array_equal(s[at], to)
        # the host reader takes the same stream for valid, and writes the last entry's byte where the deltas sum to
        last = sum(deltas)
        if last < 2**64 - 1:  # (an entry at 2^64 - 1 has no end above it)
            assert P.apply_diff_bytes(b"\xa5" if to[-1] != 0xA5 else b"\x5a", stream, base_offset=last) == bytes([to[-1]])
