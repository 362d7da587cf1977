"""Shared by the device text parser's token tests (test_textparse_cpu.py, test_gpu_textparse_tokens.py): decimal strings for
f32_from_text (csrc/f32_text.h) with the lines that carry them to each place the kernel converts a number, lines whose namespace in
force crosses a group of 64 tokens, lines at the token caps, start alignments, feature names for the hash and namespace maps for the
name table.  Every generator is deterministic; lines are bytes without their newline.  Nothing here needs a GPU."""
import ctypes
import functools
import math
import random
from fractions import Fraction

import numpy as np

CSV = "A,fa\nBb,fb\nC,fc\nDdd,fd\nE,fe\nF,ff,f32\n_namespace_skip_prefix,2\n"  # tests/test_gpu_textparse.py's map

SEED = 20250117

# ---------------------------------------------------------------- numbers
IMPORTANCE, NS_WEIGHT, FEATURE_WEIGHT, F32_VALUE = range(4)
POSITIONS = ("importance", "namespace weight", "feature weight", "f32 value")
DOUBTFUL = ("truncated midpoints", "20 digits", "far exponent near a midpoint")  # families built to hold unproven members too


def _random_decimal(rng, max_digits=19, max_exp=40):
    nd = rng.randint(1, max_digits)
    ds = "".join(rng.choice("0123456789") for _ in range(nd))
    if rng.random() < 0.6:
        k = rng.randint(0, nd)
        ds = ds[:k] + "." + ds[k:]
    if rng.random() < 0.5:
        ds += rng.choice("eE") + rng.choice(["", "+", "-"]) + "%02d" % rng.randint(0, max_exp)
    if rng.random() < 0.3:
        ds = rng.choice("+-") + ds
    return ds


def _sci_digits(x, n):
    """the first n significant decimal digits of the positive Fraction x, truncated, and its decimal exponent"""
    e = math.floor(math.log10(x))
    while Fraction(10) ** e > x:
        e -= 1
    while Fraction(10) ** (e + 1) <= x:
        e += 1
    scaled = x * Fraction(10) ** (n - 1 - e)
    return str(scaled.numerator // scaled.denominator), e


def _sci(digits, e):
    return f"{digits[0]}.{digits[1:]}e{e}" if len(digits) > 1 else f"{digits}e{e}"


def _midpoint(u):
    """the midpoint of the floats with bits u and u + 1"""
    a = Fraction(float(np.uint32(u).view(np.float32)))
    b = Fraction(float(np.uint32(u + 1).view(np.float32)))
    return (a + b) / 2


def _bits_of(lo, hi):
    return int(np.float32(lo).view(np.uint32)), int(np.float32(hi).view(np.uint32))


def number_families(seed):
    """name -> decimal strings"""
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    fam = {}
    fam["random, 19 digits"] = [_random_decimal(rng) for _ in range(9000)]
    fam["random, 9 digits"] = [_random_decimal(rng, max_digits=9, max_exp=20) for _ in range(6000)]

    out = []
    for u in nrng.integers(0x00800000, 0x7f000000, size=500, dtype=np.uint32):
        mid = _midpoint(int(u))
        for n in (15, 16, 17, 19):
            out.append(_sci(*_sci_digits(mid, n)))
    fam["truncated midpoints"] = out

    out = []
    for u in nrng.integers(0x00800000, 0x7f000000, size=300, dtype=np.uint32):
        out.append(_sci(*_sci_digits(_midpoint(int(u)), 20)))  # the 20th digit is dropped: never far enough from the midpoint
    for _ in range(300):
        ds = rng.choice("123456789") + "".join(rng.choice("0123456789") for _ in range(19))
        k = rng.randint(1, 20)
        out.append(ds[:k] + "." + ds[k:] + rng.choice(["", "e-7", "E12", "e+3"]))
    fam["20 digits"] = out

    # |decimal exponent| > 22 leaves Clinger's fast path: 19 digits of a small float's midpoint (e < -22), 16 digits of a large one's
    # (e = 23); each once as truncated (within the window) and once with its 13th digit moved (3 orders of magnitude outside it)
    out = []
    lo, hi = _bits_of(1e-25, 1e-6)
    for u in nrng.integers(lo, hi, size=150, dtype=np.uint32):
        d, e = _sci_digits(_midpoint(int(u)), 19)
        out += [f"{d}e{e - 18}", f"{int(d) + 10 ** 6}e{e - 18}"]
    lo, hi = _bits_of(1.0001e38, 3.4e38)
    for u in nrng.integers(lo, hi, size=150, dtype=np.uint32):
        d, e = _sci_digits(_midpoint(int(u)), 16)
        out += [f"{d}e{e - 15}", f"{int(d) + 10 ** 3}e{e - 15}"]
    fam["far exponent near a midpoint"] = out

    # midpoints that are exact: an odd 25-bit M over 2^k is M * 5^k / 10^k, and M * 5^k < 2^53 up to k = 12
    out = ["16777217", "33554434", "1677721.7e1", "167772170e-1"]
    for j in range(300):
        M = rng.randrange(1 << 24, 1 << 25) | 1
        form = j % 3
        k = 1 + (j // 3) % (12 if form < 2 else 6)  # M * 5^6 * 1000 is still below 2^53
        m = str(M * 5 ** k)
        if form == 0:
            out.append(f"{m}e-{k}")
        elif form == 1:
            out.append(m[:-k] + "." + m[-k:])
        else:
            out.append(f"{m}000E-{k + 3:02d}")
    fam["exact midpoints"] = out

    p53 = 1 << 53
    out = ["1234567890123456789", "12345678901234567890", "1.234567890123456789", "1.2345678901234567891", "9999999999999999999",
           "99999999999999999999", "0.9999999999999999999", "0.99999999999999999999"]
    for m in (p53 - 1, p53, p53 + 1):
        out += [str(m), f"{m}e-5", f"{m}e5", f"{m}e22", f"{m}e-22", f"{m}e-23", f"0.{m}"]
    out += ["1e22", "3e-22", "1e23", "7e-23", "123456789e22", "123456789e23", "123456789e-22", "123456789e-23", "1234567e-44", "1234567e-45",
            "12345678901234567e-44", "12345678901234567e-45", "1e44", "1e45", "0.0001e48", "0.00001e49", "1e-44", "1e-45", "1.4e-45", "0.7e-45",
            "1.17549435e-38", "1.1754943e-38", "1.1754944e-38", "1.17549428e-38", "1.1754942e-38", "1.17549421e-38", "1.175494350822287508e-38",
            "3.4028234e38", "3.4028235e38", "3.4028236e38", "3.40282357e38", "3.4028235677973366e38", "3.4028235677973367e38",
            "340282346638528859811704183484516925440", "340282356779733661637539395458142568448", "340282356779733661637539395458142568447",
            "340282366920938463463374607431768211456", "340282366920938463463374607431768211455", "1e38", "1e39", "4e38",
            "000.5000", "0." + "0" * 30 + "1", "0" * 25 + "1", "1" + "0" * 25, "1.5" + "0" * 30, "0.000", "00", "0e5", "0e99999", "0.0e-99999",
            ".5", "5.", "+1", "-0", "-0.0e5", "-1e-50", "+.5e-0", "-5.e1", "1E+05", "1e+05", "1E-05", "1e0005", "2.5", "-2.5", "-1", "1.0", "1"]
    fam["edges"] = out

    # outside the grammar, or the host's by rule: the lines stop or go to the host exactly as the host parser says
    fam["host"] = ["inf", "-Infinity", "NaN", "NONE", "1e", ".", "1_0", "0x1", "1:1", "+inf", "INF", "-inf", "nan", "infinity", "e5", "+", "-", "1e+",
                   "1.2.3", "--1", "none", "1f", "1e5.0", "1:1.0", "2:1", "1.5:NONE"]
    return fam


def numbers(seed):
    return [s for v in number_families(seed).values() for s in v]


_libc = None


def _strtof(s):
    global _libc
    if _libc is None:
        _libc = ctypes.CDLL("libc.so.6")
        _libc.strtof.restype = ctypes.c_float
        _libc.strtof.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    return _libc.strtof(s.encode(), None)


@functools.lru_cache(maxsize=None)
def usable(s):
    """the kernel's number_dev on the host compilation of f32_from_text: True when the device may use the string, False when the host
    parses it (NONE, unproven, not finite), None when it is outside the grammar (the host parser's error)"""
    from fwumious_wabbit_amd import capi
    from fwumious_wabbit_amd.feed import f32_from_text
    if s == "NONE":
        return False
    try:
        v, proven = f32_from_text(s)
    except capi.FwgpuError:
        return None
    return bool(proven and np.isfinite(v))


def _verdict(pos, s):
    """-> True (the device takes the line), False (the host parses it), None (the host parser stops with an error)"""
    if pos == F32_VALUE:  # the token is ab<S>: the first ':' splits value and weight
        val, colon, w = s.partition(":")
        ok = True if val == "" else usable(val)
        if ok is None:
            return None
        if colon:  # an f32 feature's weight must multiply to 1.0
            wok = usable(w)
            if wok is None or w == "NONE" or _strtof(w) != 1.0:
                return None
            ok = ok and wok
        return ok
    ok = usable(s)
    if ok is None:
        return None
    if pos == IMPORTANCE and s != "NONE" and _strtof(s) < 0.0:
        return None  # "Example importance cannot be negative"
    return ok


def number_line(pos, s, label=True):
    if pos == IMPORTANCE:
        return f"1 {s} |A a".encode()
    if pos == NS_WEIGHT:
        return (("1 " if label else "") + f"|A:{s} a b").encode()
    if pos == FEATURE_WEIGHT:
        return (("-1 " if label else "") + f"|A a:{s} |C c").encode()
    return f"|F ab{s}".encode()


def number_lines(nums, label=True, max_negative_importances=64):
    """Each string in the places where the kernel calls number_dev, one line each: importance (labelled lines only), namespace weight,
    feature weight, f32 value.  -> (lines, pos, takes, stops): takes[i] is whether the device may take lines[i], predicted from the host
    compilation of f32_from_text alone; stops are the (line, pos) the host parser ends at with an error, kept out of `lines` so that a
    buffer of them parses to its end.  A negative importance is such a stop whatever its digits (the same digits are converted in
    the three other places): only the first `max_negative_importances` of them are listed."""
    lines, poss, takes, stops = [], [], [], []
    n_neg = 0
    for s in nums:
        for pos in range(4):
            if pos == IMPORTANCE and not label:
                continue
            v = _verdict(pos, s)
            if v is None:
                if pos == IMPORTANCE and usable(s) is not None:
                    n_neg += 1
                    if n_neg > max_negative_importances:
                        continue
                stops.append((number_line(pos, s, label), pos))
                continue
            lines.append(number_line(pos, s, label))
            poss.append(pos)
            takes.append(v)
    return lines, poss, takes, stops


# ---------------------------------------------------------------- token groups
def count_tokens(line):
    """token starts by the kernel's rule: a non-space byte after a space, from the first '|' (the line without its newline)"""
    pos = line.find(b"|")
    if pos < 0:
        return 0
    return sum(1 for b in range(pos, len(line)) if line[b] != 0x20 and (b == pos or line[b - 1] == 0x20))


def _feat(j):
    return f"x{j}:0.5" if j % 5 == 4 else f"x{j}"


def _f32feat(j):
    return "ab%d.5" % (j % 9) if j % 7 else "ab1.5"


LABELS = ("", "1 ", "-1 0.5 ")
GROUP_EDGES = (0, 1, 62, 63, 64, 65, 126, 127, 128, 191, 192)
GROUP_KINDS = (("|A:2.5", "|C"), ("|Bb:0.5", "|C"), ("|F", "|C"), ("|A", "|A"))  # (the namespace token under test, the one in force before it)


def group_lines():
    """-> [(line, number of tokens)]: the namespace in force, its weight and its f32 flag carried from one group of 64 tokens to the next"""
    out = []

    def add(toks):
        out.append(((LABELS[len(out) % 3] + " ".join(toks)).encode(), len(toks)))

    # a namespace token at index i, features up to the end of the group after the next edge and six more
    for i in GROUP_EDGES:
        for ns, before in GROUP_KINDS:
            total = (i // 64 + 2) * 64 + 6
            toks = []
            for j in range(total):
                if j == i:
                    toks.append(ns)
                elif j == 0:
                    toks.append(before)
                elif j > i and ns == "|F":
                    toks.append(_f32feat(j))
                else:
                    toks.append(_feat(j))
            if len(out) % 2:
                toks += ["|E", "tail"]
            add(toks)
    # two and three rounds carry with no namespace token
    for nfeat in (130, 200):
        add(["|Bb:0.5"] + [_feat(j) for j in range(nfeat)])
        add(["|A", "q", "|Ddd:3", "|F"] + [_f32feat(j) for j in range(nfeat)])
    # the first feature of a namespace is the last token of a group, its second the first of the next: promoted, weighted, under a weight
    for edge in (64, 128):
        for ns, first in (("|C", "p"), ("|C", "p:2"), ("|Bb:0.5", "p"), ("|C:1.0", "p:1")):
            toks = ["|A"] + [_feat(j) for j in range(edge - 3)] + [ns, first, "q", "|E", "r", "s:3"]
            assert toks[edge - 1] == first and toks[edge] == "q"
            add(toks)
    # namespace tokens in lanes 10, 40 and 63 of one group and none in the next
    for base in (0, 64):
        toks = ["|A"] + [_feat(j) for j in range(1, base + 141)]
        toks[base + 10], toks[base + 40], toks[base + 63] = "|Bb:0.5", "|C", "|A:2.5"
        add(toks)
    return out


def cap_lines(cap, max_bytes, min_bytes=0):
    """-> [(line, tokens)] with cap - 1, cap and cap + 1 tokens: '|A' and features of the least width that makes every line (with its
    newline) longer than min_bytes; all of them at most max_bytes long"""
    width = 1
    while 2 + (cap - 2) * (width + 1) + 1 <= min_bytes:
        width += 1
    alpha = "abcdefghijklmnopqrstuvwxyz0123456789"
    out = []
    for ntok in (cap - 1, cap, cap + 1):
        feats = [alpha[j % 36] + alpha[(j // 36) % 36] * (width - 1) for j in range(ntok - 1)]
        line = ("|A " + " ".join(feats)).encode()
        assert min_bytes < len(line) + 1 <= max_bytes
        out.append((line, ntok))
    return out


def sized_line(size, tok=21):
    """a plain line that is `size` bytes long with its newline, in tokens of `tok` bytes"""
    body = "|A"
    while len(body) + 1 + tok + 1 <= size - 1:
        body += " " + "x" * (tok - 3) + "%03d" % (len(body) % 997)
    pad = size - 1 - len(body)
    body += " " + "y" * (pad - 1) if pad >= 2 else "z" * pad
    assert len(body) == size - 1
    return body.encode()


def aligned(text_line, o):
    """whole plain lines, newlines included, whose total length is o modulo 16: put in front of `text_line` at the start of a buffer they
    make it start at offset o of a 16-byte granule"""
    first = b"-1 |Bb b c\n"
    k = (o - len(first) - 7) % 16  # "1 |A " + name + "\n" is 6 + len(name) bytes, the name at least one
    prefix = first + b"1 |A " + b"p" * (k + 1) + b"\n"
    assert len(prefix) % 16 == o and text_line[:1] != b"\n"
    return prefix


# ---------------------------------------------------------------- feature names
def names(seed):
    """feature names (bytes) for murmur3: every length 0 .. 70 from the bytes 0x21 .. 0xff without ':' (a '|' never first), names of
    bytes >= 0x80 only, '|' inside and at the end, NONE, and names that differ only in their last 1, 2 or 3 bytes"""
    rng = random.Random(seed)
    pool = [b for b in range(0x21, 0x100) if b != ord(":")]
    out = []
    for n in range(71):
        nm = bytes(rng.choice(pool) for _ in range(n))
        if nm[:1] == b"|":
            nm = b"!" + nm[1:]
        out.append(nm)
    for n in (1, 2, 3, 4, 5, 7, 8, 33):
        out.append(bytes(rng.randrange(0x80, 0x100) for _ in range(n)))
    out += [b"a|b", b"ab|", b"a||b|", b"x|A", "fé|日".encode(), b"NONE", b"NONE1", b"none"]
    for tail in (b"a", b"b", b"\xff", b"xa", b"xb", b"ya", b"\x80\xff", b"xya", b"xyb", b"xza", b"zya", b"\xff\xfe\xfd"):
        out.append(b"basename" + tail)  # 8 bytes in whole words, then a tail of 1, 2 or 3
    return out


def name_lines(nms):
    """-> (lines, takes): each name as a single feature, as the first of a promoted pair and as a weighted feature, under two namespaces
    (two seeds); the empty name only as ':2'.  A NONE weight is the host's."""
    lines, takes = [], []
    for k, nm in enumerate(nms):
        other = nms[(k + 1) % len(nms)] or b"o"
        if nm:
            lines += [b"1 |A " + nm, b"|Bb " + nm, b"-1 |Bb " + nm + b" " + other, b"1 2 |A " + other + b" " + nm + b" |C " + nm]
            takes += [True] * 4
        lines += [b"1 |A " + nm + b":2", b"|Bb:0.5 " + nm + b":2 " + nm + b":3"]
        takes += [True] * 2
        if k % 16 == 0:
            lines.append(b"1 |C " + nm + b":NONE q")
            takes.append(False)
    return lines, takes


# ---------------------------------------------------------------- namespace maps
def fnv1a(name):
    h = 2166136261
    for b in name:
        h = ((h ^ b) * 16777619) & 0xffffffff
    return h


def ns_table(ns_names):
    """fwgpu_parser::build_ns_table (csrc/parser_types.h, uploaded as it is by text_parser.cpp where hp.ns_mask is read): the least power
    of two that is at least 16 and four times the entries, FNV-1a of the name's bytes, linear probing.
    -> (mask, {name: (home slot, slot)})"""
    cap = 16
    while cap < 4 * len(ns_names):
        cap <<= 1
    mask = cap - 1
    used, where = {}, {}
    for nm in ns_names:
        home = slot = fnv1a(nm.encode()) & mask
        while slot in used:
            slot = (slot + 1) & mask
        used[slot] = nm
        where[nm] = (home, slot)
    return mask, where


FIXED_NS = ["A", "AA", "AAA", "B", "Bb", "Bbb", "C", "E", "x", "y", "z", "0", "9", "_", "-", "~", "!", "#", "xy", "yx", "zz", "a1", "1a",
            "é", "ß", "éé", "日", "日本", "日本語", "Aé", "\U0001f600", "Ddd", "Dd", "D", "longer_name_of_a_namespace"]
F32_NS = ["F", "FF", "µ"]
BIG_MASK = 1023  # the table of 255 and 256 names


def big_map(n):
    """-> (csv, names, f32 names): n namespaces with one-byte, two-byte and UTF-8 names, names that are prefixes of others, three f32
    namespaces and a skip prefix of 2.  From 201 names on, three of them have the table's last slot (1023 for up to 256 names) as their
    home: a probe chain of three that wraps round the mask."""
    nms = (FIXED_NS + F32_NS)[:n]
    chain, j = [], 0
    while len(chain) < 3:
        c = "k%d" % j
        if fnv1a(c.encode()) & BIG_MASK == BIG_MASK:
            chain.append(c)
        j += 1
    j = 0
    while len(nms) < n - 3:
        c = "n%d" % j
        j += 1
        if fnv1a(c.encode()) & BIG_MASK not in (BIG_MASK, 0, 1, 2):  # the chain's slots stay the chain's
            nms.append(c)
    nms += chain[: n - len(nms)]
    f32 = [x for x in F32_NS if x in nms]
    csv = "".join("%s,v%d%s\n" % (nm, i, ",f32" if nm in f32 else "") for i, nm in enumerate(nms)) + "_namespace_skip_prefix,2\n"
    return csv, nms, f32


def undeclared_on_chain(nms):
    """a name the map does not have whose home slot is the first of big_map's chain: its probe walks the chain, wraps, and ends on an empty slot"""
    j = 0
    while True:
        c = "u%d" % j
        if c not in nms and fnv1a(c.encode()) & BIG_MASK == BIG_MASK:
            return c
        j += 1


def map_lines(nms, f32, seed):
    """a few hundred lines that name every namespace: each beside its neighbours in the list (a prefix beside its longer sibling, the
    chain's names together), then random picks"""
    rng = random.Random(seed)

    def toks(nm, j):
        if nm in f32:
            return ["|" + nm, "ab%d.25" % j, "cd-1e-3"][: 1 + j % 3]
        w = ":0.5" if j % 4 == 3 else ""
        return ["|" + nm + w] + ["v%d" % (j + q) + (":2" if q == 2 else "") for q in range(j % 4)]

    lines = []
    for j in range(len(nms)):
        picked = [nms[(j + q) % len(nms)] for q in range(3)]
        lines.append((LABELS[j % 3] + " ".join(t for q, nm in enumerate(picked) for t in toks(nm, j + q))).encode())
    for j in range(60):
        picked = [rng.choice(nms) for _ in range(rng.randint(1, 6))]
        lines.append((LABELS[j % 3] + " ".join(t for q, nm in enumerate(picked) for t in toks(nm, j + q))).encode())
    return lines
