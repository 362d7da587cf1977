"""The rule that lets a wave's range of the config-C learn kernel end INSIDE a field (fwumious_wabbit_amd/csrc/wave_balance.h: split_fields_on,
split_cut), checked on the CPU as test_wave_balance_cpu.py checks wave_of_field: the header is compiled into a stand-alone program that forms the eight
ranges of an example exactly as the kernel does -- the field that holds row floor(w nf / nw), then split_cut -- and beside them wave_of_field's ranges.

Held here, on the 10 000 seeded config-C examples of test_wave_balance_cpu.py and on crafted ones:
  * every row is owned once: the ranges are intervals, in wave order, with nothing between them;
  * (a) a field lies in at most two ranges; (b) the part of a cut field in the second range -- its lead -- is at most FW_SPLIT_LEAD_MAX rows, all of them
    among the range's first FW_MAXR_WIN rows (the register-kept ones);
  * a range longer than ceil(nf / nw) has a cut that fell back to a field boundary at one of its ends;
  * a cut that fell back lies where wave_of_field puts it, so an example whose cuts all fall back has wave_of_field's ranges; below the threshold of
    16 nw rows (split_fields_on) the ranges are wave_of_field's without looking further;
  * a restatement of the rule in Python gives the same ranges.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_wave_balance_cpu import HEADER_DIR, KEPT_MAX, NW, lopsided_shapes

LEAD_MAX, MAXR = 8, 20  # FW_SPLIT_LEAD_MAX, FW_MAXR_WIN of kernels.hip
MIN_ROWS = 16 * NW      # split_fields_on: kSplitMinShare rows per wave

PROGRAM = r"""
#include "wave_balance.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace fwgpu;
// argv[1]: lead_max.  stdin: one example per line: F, then F field sizes.
// stdout: per example one line: nf, then per wave: lo cnt (split rule) lo cnt (wave_of_field)
int main(int argc, char **argv) {
    const uint32_t nw = %d, lead_max = (uint32_t)atoi(argv[1]);
    unsigned F;
    while (scanf("%%u", &F) == 1) {
        std::vector<uint32_t> a(F), b(F), fld;
        uint32_t nf = 0;
        for (unsigned f = 0; f < F; ++f) {
            unsigned n;
            if (scanf("%%u", &n) != 1) return 1;
            a[f] = nf;
            nf += n;
            b[f] = nf;
            for (unsigned i = 0; i < n; ++i) fld.push_back(f);
        }
        uint32_t lo[8], hi[8], plo[8], phi[8];
        for (uint32_t w = 0; w < nw; ++w) {
            plo[w] = 0xffffffffu;
            phi[w] = 0;
        }
        for (unsigned f = 0; f < F; ++f)
            if (b[f] > a[f]) {
                const uint32_t w = wave_of_field(a[f], b[f], nw, nf);
                plo[w] = a[f] < plo[w] ? a[f] : plo[w];
                phi[w] = b[f] > phi[w] ? b[f] : phi[w];
            }
        for (uint32_t w = 0; w < nw; ++w) {
            if (split_fields_on(nw, nf)) {  // (as the kernel: the row's own field word names the field that holds it)
                uint32_t c[2];
                for (int e = 0; e < 2; ++e) {
                    const uint32_t v = w + e;
                    if (v == 0) c[e] = 0;
                    else if (v >= nw) c[e] = nf;
                    else {
                        const uint32_t f = fld[(v * nf) / nw];
                        c[e] = split_cut(a[f], b[f], v, nw, nf, lead_max);
                    }
                }
                lo[w] = c[0];
                hi[w] = c[1];
            } else {
                lo[w] = plo[w];
                hi[w] = phi[w];
            }
        }
        printf("%%u", nf);
        for (uint32_t w = 0; w < nw; ++w) {
            const uint32_t cnt = hi[w] > lo[w] ? hi[w] - lo[w] : 0, pcnt = phi[w] > plo[w] ? phi[w] - plo[w] : 0;
            printf(" %%u %%u %%u %%u", cnt ? lo[w] : 0, cnt, pcnt ? plo[w] : 0, pcnt);
        }
        printf("\n");
    }
    return 0;
}
""" % NW

CRAFTED = {
    "one_field_of_89": [4] * 12 + [89] + [4] * 17,   # three targets inside one field: all three fall back
    "one_field_of_89_first": [89] + [4] * 29,
    "all_fields_of_one_feature": [1] * 30,           # 30 rows: below the threshold
    "128_fields_of_one_feature": [1] * 128,          # every target is a boundary
    "fewer_features_than_waves": [1, 0, 1, 0, 1, 1, 1],
    "threshold_minus_1": [9, 3] * 10 + [7],          # 127 rows
    "threshold": [9, 3] * 10 + [8],                  # 128 rows: targets 16, 32, 64, 80, 112 lie 4 or 8 rows into a field of 9 (leads 5 and 1), 48 and 96 are boundaries
    "threshold_plus_1": [9, 3] * 10 + [9],           # 129 rows
    "lead_of_exactly_the_most": [25 - 3, 3 + LEAD_MAX] + [25] * 6 + [17],  # 200 rows, target 25 is 3 rows into a field of 11: lead 8
    "lead_one_too_long": [25 - 3, 3 + LEAD_MAX + 1] + [25] * 6 + [16],
    "field_of_two_targets": [20, 40] + [20] * 7,     # 200 rows: targets 25 and 50 inside [20, 60)
}


def _examples():
    rng = np.random.default_rng(20240612)
    ex = [list(1 + rng.poisson(5.67, size=30)) for _ in range(10000)]  # the sample of test_wave_balance_cpu.py (profiles/r07_wave_balance.txt, section 0)
    ex += list(lopsided_shapes().values())
    ex += list(CRAFTED.values())
    return ex


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/bin/hipcc"
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("field_split")
    src, exe = d / "split.cpp", d / "split"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-x", "c++", f"-I{HEADER_DIR}", str(src), "-o", str(exe)], check=True)
    ex = _examples()
    text = "".join(f"{len(e)} " + " ".join(str(int(n)) for n in e) + "\n" for e in ex)

    def run(lead_max):
        out = subprocess.run([str(exe), str(lead_max)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(ex)
        return [np.array(l.split(), dtype=np.int64) for l in out]

    return ex, run


@pytest.fixture(scope="module")
def answers(program):
    ex, run = program
    return ex, run(LEAD_MAX)


def _bounds(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _field_of_row(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


def _py_cut(sizes, w, nf, lead_max):
    """the rule restated: (cut, fell back)"""
    starts = _bounds(sizes)
    c = (w * nf) // NW
    f = int(_field_of_row(sizes)[c])
    a, b = int(starts[f]), int(starts[f + 1])
    if c == a:
        return a, False
    prev, nxt = ((w - 1) * nf) // NW, ((w + 1) * nf) // NW
    if prev <= a and nxt >= b and b - c <= lead_max:
        return c, False
    return (a if (a + b) * NW >= 2 * nf * w else b), True


def _ranges(r):
    w = r[1:].reshape(NW, 4)
    return int(r[0]), w[:, 0], w[:, 1], w[:, 2], w[:, 3]


def test_ranges_own_every_row_once_and_keep_both_conditions(answers):
    ex, rows = answers
    for sizes, r in zip(ex, rows):
        nf, lo, cnt, plo, pcnt = _ranges(r)
        assert nf == sum(sizes)
        pos = 0
        for v in range(NW):
            if cnt[v]:
                assert lo[v] == pos, (sizes, v)  # one interval each, in wave order, nothing between them and nothing twice
                pos += int(cnt[v])
        assert pos == nf
        if nf < MIN_ROWS:  # below the threshold: wave_of_field's ranges as they are
            assert np.array_equal(lo, plo) and np.array_equal(cnt, pcnt), sizes
            continue
        starts = _bounds(sizes)
        fld = _field_of_row(sizes)
        # (a) a field lies in at most two ranges
        owner = np.repeat(np.arange(NW), cnt)
        for f, n in enumerate(sizes):
            if n:
                assert len(set(owner[starts[f]:starts[f + 1]])) <= 2, (sizes, f)
        cuts = [_py_cut(sizes, v, nf, LEAD_MAX) for v in range(1, NW)]
        edge = [0] + [c for c, _ in cuts] + [nf]
        back = [False] + [s for _, s in cuts] + [False]
        for v in range(NW):
            # the restated rule
            assert (int(cnt[v]) == max(edge[v + 1] - edge[v], 0)) and (not cnt[v] or int(lo[v]) == edge[v]), (sizes, v)
            if not cnt[v]:
                continue
            # (b) the lead: rows of the range's first field that lie behind that field's start
            f = int(fld[lo[v]])
            lead = int(starts[f + 1] - lo[v]) if starts[f] < lo[v] else 0
            assert lead <= LEAD_MAX and lead <= min(int(cnt[v]), MAXR), (sizes, v)
            if lead:
                assert lo[v] == (v * nf) // NW and not back[v]
            # nothing longer than its share unless a cut fell back
            if cnt[v] > -(-nf // NW):
                assert back[v] or back[v + 1], (sizes, v)
        # a cut that fell back is the start of wave_of_field's range of the first wave at or behind v that has one
        for v in range(1, NW):
            if back[v]:
                nxt = [u for u in range(v, NW) if pcnt[u]]
                assert edge[v] == (int(plo[nxt[0]]) if nxt else nf), (sizes, v)
        if all(back[1:NW]):
            assert np.array_equal(lo, plo) and np.array_equal(cnt, pcnt), sizes


def test_ranges_are_wave_of_fields_when_every_cut_falls_back(program):
    """lead_max = 0: no cut may stay inside a field.  Wherever no target is a field boundary as it is, all seven cuts fall back and the ranges must be wave_of_field's."""
    ex, run = program
    rows = run(0)
    n = 0
    for sizes, r in zip(ex, rows):
        nf, lo, cnt, plo, pcnt = _ranges(r)
        if nf < MIN_ROWS:
            continue
        bounds = set(int(x) for x in _bounds(sizes))
        if any((v * nf) // NW in bounds for v in range(1, NW)):
            continue
        n += 1
        assert np.array_equal(lo, plo) and np.array_equal(cnt, pcnt), sizes
    print(f"\n{n} examples with no target on a field boundary")
    assert n >= 1000


def test_crafted_cases(answers):
    ex, rows = answers
    got = {name: _ranges(rows[len(ex) - len(CRAFTED) + i]) for i, name in enumerate(CRAFTED)}
    nf, lo, cnt, plo, pcnt = got["one_field_of_89"]
    assert nf == 205 and lo[1] == 25 and cnt[2] == 0 and lo[3] == 48 and cnt[3] == 89 and cnt[4] == 0 and lo[5] == 137  # the long field stays whole, in the wave its middle lies in; the cut in front of it is a split
    nf, lo, cnt, _, _ = got["one_field_of_89_first"]
    assert cnt[0] == 0 and cnt[1] == 89 and cnt[2] == 0 and lo[3] == 89 and lo[4] == 102
    for name in ("all_fields_of_one_feature", "fewer_features_than_waves", "threshold_minus_1"):
        nf, lo, cnt, plo, pcnt = got[name]
        assert nf < MIN_ROWS and np.array_equal(lo, plo) and np.array_equal(cnt, pcnt), name
    nf, lo, cnt, _, _ = got["128_fields_of_one_feature"]
    assert list(cnt) == [16] * 8
    nf, lo, cnt, _, _ = got["threshold"]
    assert nf == 128 and list(lo) == [16 * v for v in range(8)] and list(cnt) == [16] * 8  # five of the seven cuts lie inside a field
    nf, lo, cnt, _, _ = got["threshold_plus_1"]
    assert nf == 129 and list(lo) == [(v * 129) // 8 for v in range(8)]
    nf, lo, cnt, _, _ = got["lead_of_exactly_the_most"]
    assert nf == 200 and lo[1] == 25 and list(cnt) == [25] * 8  # 8 lead rows: still a split
    nf, lo, cnt, _, _ = got["lead_one_too_long"]
    assert nf == 200 and lo[1] == 22  # 9 rows would follow the cut: it falls back to the nearer boundary, the field's start
    nf, lo, cnt, _, _ = got["field_of_two_targets"]
    assert nf == 200 and cnt[0] == 20 and cnt[1] == 40 and lo[2] == 60 and lo[3] == 75  # both fall back: the field goes whole to wave 1, in whose share its middle, row 40, lies; the next cut is a split


def test_config_c_ranges_are_even(answers):
    """what the rule is for, on the seeded config-C sample (the figures of profiles/r08_field_split.txt, section 0)"""
    ex, rows = answers
    new_max, old_max, new_re, old_re, back, cuts, split_ex, leads = [], [], 0, 0, 0, 0, 0, []
    for sizes, r in list(zip(ex, rows))[:10000]:
        nf, lo, cnt, plo, pcnt = _ranges(r)
        new_max.append(int(cnt.max()))
        old_max.append(int(pcnt.max()))
        new_re += int(np.maximum(cnt - KEPT_MAX, 0).sum())
        old_re += int(np.maximum(pcnt - KEPT_MAX, 0).sum())
        if nf < MIN_ROWS:
            continue
        cs = [_py_cut(sizes, v, nf, LEAD_MAX) for v in range(1, NW)]
        back += sum(s for _, s in cs)
        cuts += NW - 1
        bounds = set(int(x) for x in _bounds(sizes))
        ld = [int(min(b for b in bounds if b > c) - c) for c, _ in cs if c not in bounds]
        split_ex += bool(ld)
        leads += ld
    print(f"\nlongest range per example: {np.mean(old_max):.2f} -> {np.mean(new_max):.2f} rows (largest {max(new_max)}); re-read rows per example: "
          f"{old_re / 1e4:.2f} -> {new_re / 1e4:.2f}; cuts that fell back: {100.0 * back / cuts:.2f} %; examples with a split: {split_ex}; "
          f"lead rows per example: {sum(leads) / 1e4:.2f}")
    assert np.mean(new_max) < np.mean(old_max) - 2.0
    assert new_re < old_re
