"""The device text parser (csrc/textparse.hip, csrc/f32_text.h as the device compiles it) on the inputs of text_token_cases.py: numbers
in every place the kernel converts one, the namespace in force across groups of 64 tokens, the token caps, every start alignment at the
staging sizes' edges, feature names of any bytes and namespace maps at the table's size limit.  Every comparison is equality with the
host parser (words, offsets, consumed bytes, code, message, command argument: _same of test_gpu_textparse.py); beside it every test
counts the lines the device handed to the host (DeviceVowpalParser.last_lines) against what the host compilation of f32_from_text
predicts, so that neither a device that proves less (a silent fall-back) nor one that proves more goes unnoticed."""
import random

import pytest

from fwumious_wabbit_amd import capi
from fwumious_wabbit_amd.feed import DeviceVowpalParser, VowpalParser, VwNamespaceMap
import text_token_cases as K
from test_gpu_serving_text import CTX, Ctx, _check_against_host, rig  # noqa: F401 (the fixture)
from test_gpu_textparse import CSV, _same, gen_line, pair  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

assert CSV == K.CSV


def _buffer(lines):
    return b"\n".join(lines) + b"\n"


def _parse(host, dev, lines, n_ns=6, text=None):
    """_same on the lines as one buffer that is parsed to its end -> the device's (lines, host lines)"""
    text = _buffer(lines) if text is None else text
    h = _same(host, dev, text, words_cap=len(text) + (n_ns + 16) * len(lines))
    assert h[3] == capi.OK and h[2] == len(text) and len(h[1]) == len(lines) + 1
    return dev.last_lines()


def _first_miscounted(host, dev, lines, takes):
    """the first line whose side is not the predicted one (a failure's message; the records are equal either way)"""
    lo, hi = 0, len(lines)  # the prefix of lo lines counts as predicted, the one of hi lines does not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _parse(host, dev, lines[:mid]) == (mid, takes[:mid].count(False)):
            lo = mid
        else:
            hi = mid
    return lo, lines[lo], takes[lo]


# ---------------------------------------------------------------- 1. numbers
def test_numbers_in_all_four_positions(pair):
    host, dev = pair
    lines, pos, takes, stops = K.number_lines(K.numbers(K.SEED))
    for p in range(4):  # per place first, for the report: the whole buffer below is what counts
        sub = [i for i in range(len(lines)) if pos[i] == p]
        got = _parse(host, dev, [lines[i] for i in sub])
        print("%s: device reports %s, predicted %s" % (K.POSITIONS[p], got, (len(sub), sum(1 for i in sub if not takes[i]))))
    got = _parse(host, dev, lines)
    want = (len(lines), takes.count(False))
    print("all four: device reports %s, predicted %s" % (got, want))
    if got != want:
        pytest.fail("last_lines %s, predicted %s; first line on the other side: %s" % (got, want, _first_miscounted(host, dev, lines, takes)))
    # strings the host parser stops at, each in its place among plain lines
    rng = random.Random(5)
    plain = [gen_line(rng).encode() for _ in range(120)]
    for line, p in stops:
        for at in (0, 57):
            ls = list(plain)
            ls[at] = line
            h = _same(host, dev, _buffer(ls))
            assert h[3] == capi.ERR_PARSE and len(h[1]) == at + 1, line
            assert dev.last_lines() == (at + 1, 0), line  # the plain lines before it were the device's; the stop itself is no record


# ---------------------------------------------------------------- 2. token groups
def test_namespace_in_force_across_token_groups(pair):
    host, dev = pair
    lines = [line for line, _ in K.group_lines()]
    assert _parse(host, dev, lines) == (len(lines), 0)
    for line in lines:  # one by one, so that a failure names its line
        assert _parse(host, dev, [line]) == (1, 0), line[:80]
        prefix = K.aligned(line, 9)
        assert _parse(host, dev, [None] * 3, text=prefix + line + b"\n") == (3, 0), line[:80]


# ---------------------------------------------------------------- 3. token caps
@pytest.mark.parametrize("cap,max_bytes,min_bytes", [
    (512, 4096, 0),  # kShortTok of csrc/textparse.hip: lines up to kShortStage = 4096 bytes
    (4096, 65536, 4096),  # kLongTok: lines up to kLongStage = 65536 bytes
], ids=["short", "long"])
def test_token_caps(pair, cap, max_bytes, min_bytes):
    host, dev = pair
    (below, _), (at, _), (above, _) = K.cap_lines(cap, max_bytes, min_bytes)
    assert _parse(host, dev, [below]) == (1, 0)
    assert _parse(host, dev, [at]) == (1, 0)  # at the cap the line stays on the device
    assert _parse(host, dev, [above]) == (1, 1)  # beyond it the host takes it
    if cap == 512:  # kShortTok + 1 tokens in more than kShortStage bytes: the long kernel's, far below its cap
        line, ntok = K.cap_lines(514, 65536, 4096)[0]
        assert ntok == 513 and len(line) + 1 > 4096
        assert _parse(host, dev, [line]) == (1, 0)
    assert _parse(host, dev, [below, above, at, at, above]) == (5, 2)


# ---------------------------------------------------------------- 4. start alignments
@pytest.mark.parametrize("size", [4095, 4096, 4097, 65535, 65536, 65537])
def test_start_alignments_at_the_stage_edges(pair, size):
    """the line (`size` bytes with its newline) at each of the sixteen offsets within a 16-byte granule"""
    host, dev = pair
    line = K.sized_line(size)
    n_host = 1 if size > 65536 else 0  # kLongStage counts the newline
    for o in range(16):
        prefix = K.aligned(line, o)
        text = prefix + line + b"\n-1 |Bb b c\n"
        assert (len(prefix) & 15) == o and text[len(prefix) + size - 1: len(prefix) + size] == b"\n"
        assert _parse(host, dev, [None] * 4, text=text) == (4, n_host), o
        assert _parse(host, dev, [None] * 4, text=text[:-1]) == (4, n_host), o  # the last line's last byte is ignored
        assert _parse(host, dev, [None] * 3, text=text[:-11]) == (3, n_host), o  # the line last, with its newline ...
        if size <= 65536:
            assert _parse(host, dev, [None] * 3, text=text[:-12]) == (3, 0), o  # ... and without
    # (the line of 65537 bytes without its newline is one of 65536: the device's, compared below)
    if size > 65536:
        assert _parse(host, dev, [None] * 3, text=K.aligned(line, 5) + line) == (3, 0)


# ---------------------------------------------------------------- 5. feature names
def test_feature_names(pair):
    host, dev = pair
    lines, takes = K.name_lines(K.names(K.SEED))
    assert _parse(host, dev, lines) == (len(lines), takes.count(False))
    for line, take in zip(lines, takes):
        assert _parse(host, dev, [line]) == (1, 0 if take else 1), line


# ---------------------------------------------------------------- 6. namespace table
@pytest.mark.parametrize("n", [255, 256, 257])
def test_namespace_table_sizes(n):
    csv, nms, f32 = K.big_map(n)
    vw = VwNamespaceMap(csv)
    host, dev = VowpalParser(vw), DeviceVowpalParser(vw)
    lines = K.map_lines(nms, f32, n)
    # up to kTextMaxNamespaces = 256 slot words the device takes every line; a larger map is the host's whole
    assert _parse(host, dev, lines, n_ns=n) == (len(lines), 0 if n <= 256 else len(lines))
    und = K.undeclared_on_chain(nms)
    ls = lines[:20] + [("1 |A a |%s b" % und).encode()] + lines[20:40]
    text = _buffer(ls)
    h = _same(host, dev, text, words_cap=len(text) + (n + 16) * len(ls))
    assert h[3] == capi.ERR_PARSE and len(h[1]) == 21 and ("not predeclared in vw_namespace_map.csv: " + und) in h[4]
    dev.close()
    host.close()


# ---------------------------------------------------------------- 7. candidate mode
def test_candidate_mode_sees_the_same_numbers_and_groups(rig):
    """fwgpu_text_parser_parse_candidates reports the side per line: by_host against the prediction"""
    vw, mi, re, fbt, host, dev = rig
    ctx = Ctx(host, re, fbt, CTX)
    fams = K.number_families(K.SEED)
    nums = K.numbers(K.SEED)[::300] + fams["host"][:9] + fams["truncated midpoints"][:8]
    lines, pos, takes, stops = K.number_lines(nums, label=False)
    assert 190 <= len(lines) + len(stops) <= 260 and takes.count(False) >= 12 and takes.count(True) >= 100 and len(stops) >= 10
    lines += [line for line, _ in stops]  # an error is a line with a code here, and the host's
    takes += [False] * len(stops)
    groups = [line for line, _ in K.group_lines() if line[:1] == b"|"]
    assert len(groups) >= 15
    lines += groups
    takes += [True] * len(groups)
    info = _check_against_host(host, dev, fbt, ctx, [l + b"\n" for l in lines])
    assert info["by_host"].tolist() == [0 if t else 1 for t in takes]
    assert dev.last_lines() == (len(lines), takes.count(False))
    assert (info["code"] != capi.OK).sum() == len(stops)
    ctx.cache.close()
