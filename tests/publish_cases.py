"""Inputs shared by the tests of the byte diff of published inference models (tests/test_gpu_publish_diff.py): byte patterns placed on the
kernels' tile edges, and small trained models with their quantiser extremes pinned."""
import numpy as np

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import capi
from fwumious_wabbit_amd.feed import VwNamespaceMap
from helpers import make_pair

VW6 = "".join(f"A{i},ns{i}\n" for i in range(6))
# (base_offset, prev_index): the start of a file, an odd offset, and indices that cross 32 bits on a tiny array
OFFSETS = ((0, 0), (12345, 0), (2**32 - 100, 2**32 - 4096))


def lengths(tile):
    return (0, 1, 15, 16, 17, tile - 1, tile, tile + 1, 3 * tile + 5)


def patterns(n, tile, seed=0):
    """[(name, a, b)] of n bytes each; the differing positions of every pattern that fits n"""
    rng = np.random.default_rng(seed + n)
    a = rng.integers(0, 256, size=n, dtype=np.uint8)

    def at(positions):
        b = a.copy()
        b[list(positions)] ^= rng.integers(1, 256, size=len(positions), dtype=np.uint8)  # (never the same byte)
        return b

    out = [("none", a, a.copy()), ("all", a, a ^ rng.integers(1, 256, size=n, dtype=np.uint8))]
    if n >= 1:
        out += [("first", a, at([0])), ("last", a, at([n - 1]))]
    if n > tile:
        out.append(("tile-edge-pair", a, at([tile - 1, tile])))
    for density in (1e-3, 0.5):
        b = a.copy()
        hit = rng.random(n) < density
        b[hit] ^= rng.integers(1, 256, size=int(hit.sum()), dtype=np.uint8)
        out.append((f"random-{density}", a, b))
    return out


def carried_prev(tile):
    """one difference in tile 0 and the next 40 tiles on, only empty tiles between: prev is carried across them"""
    n = 41 * tile + 7
    a = np.random.default_rng(41).integers(0, 256, size=n, dtype=np.uint8)
    b = a.copy()
    b[[5, 40 * tile + 3]] ^= 0x5A
    return a, b


def long_gap(tile):
    """differences at 1 and n - 1, at least 2^21 apart: a 4-byte varint"""
    n = 2**21 + tile + 3
    a = np.random.default_rng(21).integers(0, 256, size=n, dtype=np.uint8)
    b = a.copy()
    b[[1, n - 1]] ^= 0xFF
    return a, b


def vwmap():
    return VwNamespaceMap(VW6)


def records(n, first=0):
    return fw.synth_records(6, 1.0, 1.1, 3000, 0.2, 31, first, n)


def train(re, mi, recs, off):
    b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
    re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
    b.close()


def model(opt=fw.Optimizer.AdagradLUT, bits=14, n=300, nn=False):
    """6 fields, k = 4, tables of 2^bits entries, trained on n examples"""
    mi, _, _ = make_pair(6, 4, bits, bits, opt, lr=0.05, ffm_lr=0.05)
    if nn:
        mi.nn_layers = [dict(width="9", activation="relu"), dict(width="5", activation="relu", init="xavier")]
    re = fw.Regressor(mi)
    train(re, mi, *records(n))
    return mi, re


def untouched_ffm_weights(mi, n_examples, count=2):
    """indices of FFM weights that none of the first n_examples examples touches: their AdaGrad accumulators stay at the initial value"""
    probe = fw.Regressor(mi)
    acc0 = probe.table_read(capi.TABLE_FFM_ACC)
    train(probe, mi, *records(n_examples))
    idle = np.nonzero(probe.table_read(capi.TABLE_FFM_ACC) == acc0)[0]
    probe.close()
    assert idle.size >= count
    return [int(i) for i in idle[:: max(1, idle.size // count)][:count]]


def pinned_model(first=300, more=40, bits=16):
    """(mi, re, more_records): a model trained on `first` examples whose FFM extremes are +1 and -1 in two weights that neither those nor the
    next `more` examples touch -- the quantiser's 8-byte header then stays put between the two publishes by construction"""
    mi, re = model(bits=bits, n=first)
    lo, hi = untouched_ffm_weights(mi, first + more)
    w = re.table_read(capi.TABLE_FFM_W)
    assert np.abs(w).max() < 1.0
    re.table_write(capi.TABLE_FFM_W, [1.0], offset=hi)
    re.table_write(capi.TABLE_FFM_W, [-1.0], offset=lo)
    return mi, re, records(more, first=first)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def predictions(re, mi, recs, off):
    """predictions per (batch kind, mode): entry and record batches, both modes"""
    fbt = fw.FeatureBufferTranslator(mi)
    out = []
    for as_records in (False, True):
        b = re.record_batch(fbt, recs, off) if as_records else re.batch_from_records(fbt, recs, off)
        for mode in (capi.MODE_HOGWILD, capi.MODE_SEQUENTIAL):
            re.learn_batch(b, mode, False)
            out.append(b.predictions().copy())
        b.close()
    return np.stack(out)
