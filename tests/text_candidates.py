"""Shared by the serving-from-text tests: generated candidate lines (the plain-example generator of tests/test_gpu_textparse.py without a
label) and the four adjustments that turn a line's stand-alone record into fwgpu_parser_parse_candidate's candidate-only record."""
import ctypes as C

import numpy as np

from fwumious_wabbit_amd import capi

CSV = "A,fa\nBb,fb\nC,fc\nDdd,fd\nE,fe\nF,ff,f32\nG,fg\n_namespace_skip_prefix,2\n"
CAT = ["A", "Bb", "C", "Ddd", "E"]
ALPHA = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_-"
NO_FEATURES = 0x80000000
WEIGHTS = ["0.5", "2", "1.25", "0.333333", "12.5", "1e-3", "3", "1.0", "0.000125", "7.5e2"]  # numbers the device proves correctly rounded


def _name(rng, lo=1, hi=21):
    return "".join(rng.choice(ALPHA) for _ in range(rng.randint(lo, hi)))


def _weight(rng):
    return rng.choice(WEIGHTS)


def gen_candidate(rng, namespaces=None, f32_nan=True):
    """a plain label-free line: starts with '|', declared namespaces, proven weights -- everything the kernel takes itself"""
    namespaces = namespaces or CAT + ["F"]
    sp = lambda: " " * rng.randint(1, 3)  # noqa: E731
    toks = []
    nss = [rng.choice(namespaces) for _ in range(rng.randint(1, 5))]
    if rng.random() < 0.2:
        nss.append(nss[0])  # named twice: starts over, the first run's words stay behind
    for ns in nss:
        if ns == "F":
            toks.append("|F")
            for _ in range(rng.randint(0, 2)):
                toks.append("ab" + (_weight(rng) if (rng.random() < 0.8 or not f32_nan) else ""))
            continue
        toks.append("|" + ns + (":" + _weight(rng) if rng.random() < 0.2 else ""))
        for _ in range(rng.choice([0, 1, 1, 1, 2, 3])):  # empty, single in place, promoted by a second feature
            toks.append(_name(rng) + (":" + _weight(rng) if rng.random() < 0.2 else ""))
    out = toks[0]
    for t in toks[1:]:
        out += sp() + t
    return out


def adjusted(stand, ctx_rec, n_ns):
    """the candidate-only record of a line that starts with '|', from its stand-alone record: words 1 and 2 are the context record's,
    and a slot whose merged form (a single feature: the hash; a range: moved by L0 - H) equals the context's slot word reads NO_FEATURES.
    -> (record, slots where a filled slot became NO_FEATURES)"""
    a = np.array(stand, dtype=np.uint32)
    H, L0 = 3 + n_ns, len(ctx_rec)
    a[1], a[2] = ctx_rec[1], ctx_rec[2]
    fired = 0
    for sl in range(3, H):
        w = int(a[sl])
        if w == NO_FEATURES:
            continue
        merged = w if not (w & NO_FEATURES) else w + ((L0 - H) << 16) + (L0 - H)
        if merged == int(ctx_rec[sl]):
            a[sl] = NO_FEATURES
            fired += 1
    return a, fired


def host_candidate(parser, px, line):
    """fwgpu_parser_parse_candidate on one line -> (code, record (empty for an error), is_delta)"""
    buf = np.zeros(len(line) + 65536, dtype=np.uint32)
    n, d = C.c_uint32(), C.c_int32()
    rc = capi.lib().fwgpu_parser_parse_candidate(parser.h, px.h, line, len(line), capi.ptr(buf), buf.size, C.byref(n), C.byref(d))
    if rc != capi.OK:
        return rc, buf[:0], False
    return rc, buf[: n.value].copy(), bool(d.value)

