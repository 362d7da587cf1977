"""The rule that hands an example's fields to the eight waves of the config-C learn kernel (fwumious_wabbit_amd/csrc/wave_balance.h, wave_of_field),
checked on the CPU: the header is compiled into a stand-alone program, fed field sizes, and its answers are held against the properties the kernel
relies on and against a restatement of the rule in Python: every non-empty field has one owner; a wave's fields are neighbours (its range is one
interval), the ranges tile the example in wave order, and every boundary between two waves' ranges is the field boundary NEAREST to w nf / nw.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "fwumious_wabbit_amd", "csrc")
NW, KEPT_MAX = 8, 20 + 3  # waves of a 512-thread workgroup; FW_MAXR_WIN + FW_LDS_KEEP_MAX rows of a range kept from the gather

PROGRAM = r"""
#include "wave_balance.h"
#include <cstdio>
#include <vector>
using namespace fwgpu;
// stdin: one example per line: F, then F field sizes.  stdout: per example one line: nf, then per wave: lo cnt kept
int main() {
    const uint32_t nw = %d, kept_max = %d;
    unsigned F;
    while (scanf("%%u", &F) == 1) {
        std::vector<uint32_t> a(F), b(F);
        uint32_t nf = 0;
        for (unsigned f = 0; f < F; ++f) {
            unsigned n;
            if (scanf("%%u", &n) != 1) return 1;
            a[f] = nf;
            nf += n;
            b[f] = nf;
        }
        uint32_t lo[8], hi[8], cnt[8], kept[8];
        for (uint32_t w = 0; w < nw; ++w) {
            lo[w] = 0xffffffffu;
            hi[w] = 0;
        }
        for (unsigned f = 0; f < F; ++f)
            if (b[f] > a[f]) {
                const uint32_t w = wave_of_field(a[f], b[f], nw, nf);
                if (w >= nw) return 2;
                lo[w] = a[f] < lo[w] ? a[f] : lo[w];
                hi[w] = b[f] > hi[w] ? b[f] : hi[w];
            }
        for (uint32_t w = 0; w < nw; ++w) {
            cnt[w] = hi[w] > lo[w] ? hi[w] - lo[w] : 0;
            if (!cnt[w]) lo[w] = 0;
            kept[w] = cnt[w] < kept_max ? cnt[w] : kept_max;
        }
        printf("%%u", nf);
        for (uint32_t w = 0; w < nw; ++w)
            printf(" %%u %%u %%u", lo[w], cnt[w], kept[w]);
        printf("\n");
    }
    return 0;
}
""" % (NW, KEPT_MAX)


def lopsided_shapes():
    """the per-field feature counts of tests/test_gpu_wave_balance.py's examples (F = 30)"""
    shapes = {
        "one_big_field": [60] + [1] * 29,
        "all_in_last_field": [0] * 29 + [40],
        "five_features": [1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1],
        "ten_empty_fields": [7] * 10 + [0] * 10 + [7] * 10,
        "one_thirteen": [1, 13] * 15,
        "rows_23": [23, 0, 0] * 8 + [0] * 6,
        "rows_24": [24, 0, 0] * 8 + [0] * 6,
    }
    return shapes


def _examples():
    rng = np.random.default_rng(20240612)
    ex = [list(1 + rng.poisson(5.67, size=30)) for _ in range(10000)]  # config C: 30 fields of 1 + Poisson(5.67) features
    ex += list(lopsided_shapes().values())
    ex += [[1], [3], [0, 0, 2], [200] + [0] * 29, [25] * 30, [1] * 30, [2] * 4, [9, 1] * 4]
    return ex


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/bin/hipcc"
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("wave_balance")
    src, exe = d / "split.cpp", d / "split"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-x", "c++", f"-I{HEADER_DIR}", str(src), "-o", str(exe)], check=True)
    ex = _examples()
    text = "".join(f"{len(e)} " + " ".join(str(int(n)) for n in e) + "\n" for e in ex)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(ex)
    rows = [np.array(l.split(), dtype=np.int64) for l in out]
    return ex, rows


def _py_owner(a, b, nw, nf):
    return min(((a + b) * nw) // (2 * nf), nw - 1)


def test_ranges_tile_the_example_on_the_nearest_field_boundaries(answers):
    ex, rows = answers
    for sizes, r in zip(ex, rows):
        nf, w = int(r[0]), r[1:].reshape(NW, 3)
        assert nf == sum(sizes)
        lo, cnt = w[:, 0], w[:, 1]
        starts = np.concatenate([[0], np.cumsum(sizes)])
        bounds = sorted(set(int(x) for x in starts))  # the field boundaries
        pos = 0
        for v in range(NW):
            if cnt[v] == 0:
                continue
            assert lo[v] == pos, (sizes, v)  # one interval each, in wave order, nothing between them
            pos += int(cnt[v])
            assert pos in bounds
        assert pos == nf
        # the restated rule, field by field
        for f, n in enumerate(sizes):
            if n:
                a, b = int(starts[f]), int(starts[f + 1])
                o = _py_owner(a, b, NW, nf)
                assert lo[o] <= a and b <= lo[o] + cnt[o], (sizes, f)
        # the boundary in front of wave v's range, where waves v - 1 and v both have rows, is the field boundary nearest to v nf / nw
        # (in 2 nw-ths of a row: exact); a tie goes to either neighbour
        for v in range(1, NW):
            if cnt[v] and cnt[v - 1]:
                t2 = 2 * v * nf  # 2 nw x the target
                d = abs(2 * NW * int(lo[v]) - t2)
                assert d == min(abs(2 * NW * x - t2) for x in bounds), (sizes, v)


def test_config_c_ranges_are_more_even_than_under_the_old_rule(answers):
    """what the rule is for, on the seeded config-C sample: the longest range of an example shrinks on average, and fewer rows are re-read"""
    ex, rows = answers
    new_max, old_max, new_re, old_re = [], [], 0, 0
    for sizes, r in list(zip(ex, rows))[:10000]:
        nf, w = int(r[0]), r[1:].reshape(NW, 3)
        starts = np.concatenate([[0], np.cumsum(sizes)])
        old = np.zeros(NW, dtype=np.int64)
        for f, n in enumerate(sizes):
            old[(int(starts[f]) * NW) // nf] += n
        new_max.append(int(w[:, 1].max()))
        old_max.append(int(old.max()))
        new_re += int((w[:, 1] - w[:, 2]).sum())
        old_re += int(np.maximum(old - KEPT_MAX, 0).sum())
    print(f"\nlongest range per example: {np.mean(old_max):.2f} -> {np.mean(new_max):.2f} rows; re-read rows per example: {old_re / 1e4:.2f} -> {new_re / 1e4:.2f}")
    assert np.mean(new_max) < np.mean(old_max)
    assert new_re < old_re
