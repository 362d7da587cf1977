"""The requests route on PACKED weights (fwgpu_packed_enable_caches; csrc/requests.hip), restated in numpy.  Pure numpy; nothing here touches the device.

Per shape of SHAPES -- the seven of requests_cases.SHAPES that fwgpu_model_load_packed accepts -- the case of requests_cases.case(F, k) (four caches, one
of them empty, 96 interleaved candidates) on the VALUES THE BUCKETS STAND FOR: the source tables are perturbed per weight (PERTURB_SEED), quantised and
dequantised by the reference quantiser's statements (quantization.rs:18-98 as csrc/model_file.cpp restates them), and every candidate's float64
reference is formed on the dequantised values.

build_cache() is the packed cache build kernel: T in buffer order, dcf in the order the kernel's header comment states.
planted() gives the faults a packed route can have on top of requests_cases.FAULTS."""
from types import SimpleNamespace

import numpy as np

import ffm_ref
import requests_cases as rq

SHAPES = [(6, 4), (30, 8), (20, 12), (21, 12), (16, 32), (5, 64), (30, 16)]
REFUSED = [(30, 12), (40, 16)]  # rows of more than 256 weights with ffm_k not dividing 256, and of more than 512: fwgpu_model_load_packed refuses them
assert set(SHAPES) | set(REFUSED) == set(rq.SHAPES)
PERTURB_SEED = 77
# A half-word swap exchanges NEIGHBOURS (floats 2 i and 2 i + 1 of a row).  So that such a fault cannot hide behind neighbours that share a bucket, every
# second weight of the source table is made larger by a factor drawn per weight before packing.  (Measured on the CPU: the swap is red in 69 of 96
# candidates with the perturbation -- test_packed_requests_cpu.py -- and, on cache_cases.warm_tables as they are, at 6 x 4 and 30 x 8 as well.)
PERTURB_SPAN = 0.5
PACKED_FAULTS = ("source", "swap_gather", "swap_build", "header")
NUM_BUCKETS = 65025.0

_CASES = {}


def _round_half_away(x32):
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)  # (exact: a float32 plus a half is a float64)
    return np.trunc(x + np.copysign(0.5, x)).astype(np.float32)


def quantize(w):
    """(increment, min, buckets as f16 bit patterns): quantize_header + quantize_ffm, float32 throughout"""
    w = np.asarray(w, dtype=np.float32)
    mn = np.float32(_round_half_away(w.min() * np.float32(10000.0)) / np.float32(10000.0))
    mx = np.float32(_round_half_away(w.max() * np.float32(10000.0)) / np.float32(10000.0))
    inc = np.float32((mx - mn) / np.float32(NUM_BUCKETS))
    q = _round_half_away((w - mn) / inc).astype(np.float16)
    return inc, mn, q.view(np.uint16)


def dequantize(inc, mn, buckets):
    """packed_weight (kernels.hip): the f16 pattern to float32 exactly, one multiply, one add, every operation rounded"""
    h = np.asarray(buckets, dtype=np.uint16).view(np.float16).astype(np.float32)
    return (np.float32(mn) + h * np.float32(inc)).astype(np.float32)


def swap_halves(buckets):
    """the two buckets of every 32-bit word exchanged: what a lane reads with the half-words of a word mixed up"""
    b = np.asarray(buckets, dtype=np.uint16)
    n = len(b) & ~1
    out = b.copy()
    out[0:n:2], out[1:n:2] = b[1:n:2], b[0:n:2]
    return out


def perturb(w, seed=PERTURB_SEED):
    """every odd float of the table scaled by 1 + PERTURB_SPAN * u, u uniform in [0, 1) per weight"""
    rng = np.random.default_rng(seed)
    out = np.asarray(w, dtype=np.float32).copy()
    out[1::2] *= (1.0 + PERTURB_SPAN * rng.random(len(out[1::2]))).astype(np.float32)
    return out


def wave_sum(v):
    """the butterfly of 64 partial sums: v += v[lane ^ m], m = 32 .. 1, float32"""
    v = np.asarray(v, dtype=np.float32).copy()
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = (v + v[lanes ^ m]).astype(np.float32)
    assert np.all(v.view(np.uint32) == v.view(np.uint32)[0])
    return v[0]


def build_cache(F, k, w, ctx_ffm):
    """(T [F, R], dcf [F], cnt [F]) as packed_cache_build_kernel writes them from the float32 values `w`:
    T[f][z k + kk] = sum over the features i of field z, in buffer order from 0, of w_i[f k + kk] * v_i;
    dcf[f]: lane (e0 / 4) % 64 holds floats e0 .. e0 + 3 of a row; the k / 4 lanes of the field's own slot add ((w0 w0 + w1 w1) + w2 w2) + w3 w3, times v,
    times v, per feature in buffer order from 0; the 64 lanes' sums go through the butterfly; cnt[f]: the field's features."""
    R = F * k
    w = np.asarray(w, dtype=np.float32)
    T, dcf, cnt = np.zeros((F, R), np.float32), np.zeros(F, np.float32), np.zeros(F, np.uint32)
    fld = (ctx_ffm["contra_field_index"] // k).astype(np.int64)
    assert np.all(np.diff(fld) >= 0), "the entries are ordered by field"
    for z in range(F):
        run = np.nonzero(fld == z)[0]
        cnt[z] = len(run)
        S = np.zeros(R, np.float32)  # the field's sum in the row's layout: S[f k + kk] faces field f
        lanes = np.zeros(64, np.float32)
        for i in run:
            h, v = int(ctx_ffm["hash"][i]), np.float32(ctx_ffm["value"][i])
            row = w[h:h + R]
            S = (S + (row * v).astype(np.float32)).astype(np.float32)
            for j in range(k // 4):
                e0 = z * k + 4 * j
                q = row[e0:e0 + 4]
                sq = (q * q).astype(np.float32)
                ss = np.float32(np.float32(np.float32(sq[0] + sq[1]) + sq[2]) + sq[3])
                lane = (e0 // 4) % 64
                lanes[lane] = np.float32(lanes[lane] + np.float32(np.float32(ss * v) * v))
        T.reshape(F, F, k)[:, z, :] = S.reshape(F, k)
        dcf[z] = wave_sum(lanes)
    return T, dcf, cnt


class BuiltCache:
    """requests_cases.Cache with T and dcf from build_cache (base(S) summed as there)"""

    def __init__(self, F, k, w, ctx_ffm):
        self.T, self.dcf, self.cnt = build_cache(F, k, w, ctx_ffm)
        S3 = np.ascontiguousarray(self.T.reshape(F, F, k).transpose(1, 0, 2))  # S3[z][f] = the sum of field z facing field f
        pairs = [S3[f, z] * S3[z, f] for f in range(F) for z in range(f + 1, F)]
        diag = [np.float32(0.5) * (rq._seq(S3[f, f] * S3[f, f]) - self.dcf[f]) for f in range(F)]
        self.base = rq._seq([rq._seq(np.concatenate(pairs)) if pairs else np.float32(0.0), rq._seq(diag)])


def _view(pc, w, caches_w=None):
    """the case with the gather reading `w` and the caches built from `caches_w` (default: w): what requests_cases.emulate takes"""
    cw = w if caches_w is None else caches_w
    return SimpleNamespace(F=pc.F, k=pc.k, R=pc.R, w=w, lr=pc.lr, contexts=pc.contexts,
                           emu_caches=[BuiltCache(pc.F, pc.k, cw, ctx_ffm) for _, ctx_ffm in pc.contexts])


def case(F, k):
    """requests_cases.case(F, k) on packed weights: src_w (the perturbed source table), inc / mn / buckets (its quantised block), w (the values the
    buckets stand for), cands with .ref on w; clean (the view emulate() takes); made once, shared, left unchanged"""
    if (F, k) in _CASES:
        return _CASES[(F, k)]
    cs = rq.case(F, k)
    pc = SimpleNamespace(F=F, k=k, R=F * k, cfg=cs.cfg, rs=cs.rs, sets=cs.sets, contexts=cs.contexts, lr=cs.lr, acc=cs.acc)
    pc.src_w = perturb(cs.w)
    pc.inc, pc.mn, pc.buckets = quantize(pc.src_w)
    pc.w = dequantize(pc.inc, pc.mn, pc.buckets)
    pc.cands = [SimpleNamespace(cache=x.cache, request=x.request, lr=x.lr, rest=x.rest, whole=x.whole,
                                ref=ffm_ref.predict(cs.cfg, pc.w, cs.lr, x.lr, x.whole)) for x in cs.cands]
    pc.clean = _view(pc, pc.w)
    _CASES[(F, k)] = pc
    return pc


def refreshed(pc, scale=np.float32(1.375)):
    """the source table after a training step's worth of change (every weight scaled: minimum and maximum move, so the header does) and its block"""
    src2 = (pc.src_w * scale).astype(np.float32)
    inc2, mn2, b2 = quantize(src2)
    return src2, inc2, mn2, b2


def planted(pc, fault):
    """(the view emulate() takes, the candidates' float64 references) under one of PACKED_FAULTS --
        "source"       the caches built from the SOURCE f32 weights, the gather on the buckets' values
        "swap_gather"  the predict kernel reads the two buckets of every 32-bit word exchanged (the caches are right)
        "swap_build"   the build kernel does (the gather is right)
        "header"       after a refresh: the new buckets read with the increment and minimum of the block before it (references on the new values)"""
    assert fault in PACKED_FAULTS
    refs = [x.ref for x in pc.cands]
    if fault == "source":
        return _view(pc, pc.w, pc.src_w), refs
    if fault == "swap_gather":
        return _view(pc, dequantize(pc.inc, pc.mn, swap_halves(pc.buckets)), pc.w), refs
    if fault == "swap_build":
        return _view(pc, pc.w, dequantize(pc.inc, pc.mn, swap_halves(pc.buckets))), refs
    _, inc2, mn2, b2 = refreshed(pc)
    assert (inc2, mn2) != (pc.inc, pc.mn)
    w2 = dequantize(inc2, mn2, b2)
    refs2 = [ffm_ref.predict(pc.cfg, w2, pc.lr, x.lr, x.whole) for x in pc.cands]
    return _view(pc, dequantize(pc.inc, pc.mn, b2)), refs2
