"""The rule that thins a hot FFM row's accumulator adds by the row's heat (fwumious_wabbit_amd/csrc/hot_tiers.h), checked on the CPU: the header is
compiled into a stand-alone program that is fed (base exponent, theta, initial accumulator value, accumulator) and answers with the sampling exponent,
formed exactly as the host (launch.cpp make_params: hot_tier_level) and the kernels (hot_tiers_beyond, hot_row_sample_log2) form it.

The second half emulates the config-C kernel's draw in numpy -- ((ticket * 2654435761) ^ (slot * 40503 + wave * 9973)) >> 9, masked by m - 1 -- over the
tickets and slots of tests/test_gpu_hot_tiers.py's cases: the share of turns an IDEAL implementation shows must lie inside the window that test asserts.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "fwumious_wabbit_amd", "csrc")

PROGRAM = r"""
#include "hot_tiers.h"
#include <cstdio>
using namespace fwgpu;
// stdin: one query per line: base_log2 theta initial_acc tiers_on acc (floats as hex bit patterns).  stdout: the exponent, and the three levels' bits
int main() {
    unsigned base, th, in, on, ac;
    while (scanf("%u %x %x %u %x", &base, &th, &in, &on, &ac) == 5) {
        float theta, init, acc, l[kHotTiers];
        __builtin_memcpy(&theta, &th, 4);
        __builtin_memcpy(&init, &in, 4);
        __builtin_memcpy(&acc, &ac, 4);
        for (uint32_t t = 0; t < kHotTiers; ++t) l[t] = hot_tier_level(theta, init, t, on != 0);
        unsigned lb[3];
        __builtin_memcpy(lb, l, 12);
        printf("%u %x %x %x\n", hot_row_sample_log2(base, hot_tiers_beyond(acc, l[0], l[1], l[2])), lb[0], lb[1], lb[2]);
    }
    return 0;
}
"""


def _bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/bin/hipcc"
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("hot_tiers")
    src, exe = d / "tiers.cpp", d / "tiers"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-x", "c++", f"-I{HEADER_DIR}", str(src), "-o", str(exe)], check=True)

    def f(queries):
        """queries: (base, theta, init, tiers_on, acc) -> (exponents, levels as float32 (n, 3))"""
        text = "".join(f"{int(b)} {_bits(th):x} {_bits(i):x} {int(on)} {_bits(a):x}\n" for b, th, i, on, a in queries)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        e = np.array([int(l.split()[0]) for l in out])
        lv = np.array([[int(x, 16) for x in l.split()[1:]] for l in out], dtype=np.uint32).view(np.float32)
        return e, lv

    return f


THETAS = (0.5, 0.25, 3.0)
INITS = (0.0, 1.0)  # AdagradLUT (initial value folded into its table) / AdagradFlex with ffm_init_acc_gradient = 1


@pytest.mark.parametrize("init", INITS)
@pytest.mark.parametrize("theta", THETAS)
def test_exponent_is_the_base_below_8_theta_and_steps_at_exactly_8_16_32_theta(ask, theta, init):
    up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    for base in range(7):
        lv = [np.float32(np.float32(theta) * np.float32(m) + np.float32(init)) for m in (8, 16, 32)]
        pts = [init, init + theta, up(init + theta), init + 3 * theta, init + 7.9 * theta, lv[0], up(lv[0]), init + 12 * theta, lv[1], up(lv[1]), init + 24 * theta, lv[2], up(lv[2]),
               init + 48 * theta, init + 1e6 * theta, np.inf]
        want = [0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3]  # "beyond" is strictly greater, as for the threshold itself
        e, levels = ask([(base, theta, init, 1, a) for a in pts])
        assert np.array_equal(levels[0], np.array(lv, dtype=np.float32)), (levels[0], lv)
        assert list(e) == [min(base + w, 6) for w in want], (base, list(e))
        # off: the base exponent whatever the heat; a NaN accumulator is beyond nothing
        e_off, l_off = ask([(base, theta, init, 0, a) for a in pts])
        assert list(e_off) == [base] * len(pts) and np.all(np.isinf(l_off))
        assert list(ask([(base, theta, init, 1, np.nan)])[0]) == [base]


@pytest.mark.parametrize("init", INITS)
def test_exponent_is_monotone_in_heat_and_clamped_at_6(ask, init):
    rng = np.random.default_rng(5)
    heat = np.sort(np.concatenate([rng.uniform(0, 40, 4000), 2.0 ** rng.uniform(-10, 20, 4000)])).astype(np.float32)
    for base in range(7):
        e, _ = ask([(base, 0.5, init, 1, np.float32(init) + h) for h in heat])
        assert np.all(np.diff(e) >= 0)
        assert e.min() == base and e.max() == min(base + 3, 6)
        assert np.all(e[heat < 4.0] == base)  # below 8 theta


# ---------------------------------------------------------------- the draw, emulated: what share of turns an ideal implementation shows
def draw_turns(tickets, slots, waves, m):
    """the kernel's draw for every (ticket, slot): True where the one-in-m turn comes (kernels.hip: the config-C pipelined loop)"""
    d = ((tickets.astype(np.uint64) * 2654435761) & 0xFFFFFFFF).astype(np.uint32) ^ ((slots.astype(np.uint64) * 40503 + waves.astype(np.uint64) * 9973) & 0xFFFFFFFF).astype(np.uint32)
    return ((d >> 9) & np.uint32(m - 1)) == 0


def test_an_ideal_draw_stays_inside_the_gpu_tests_window():
    """tests/test_gpu_hot_tiers.py asserts a share of turns in [0.7 / m, 1.3 / m] per tier.  Its case a has 1024 tickets x ~200 rows, a quarter of every
    third row per tier: >= 5000 units per tier on each shape, ~20 000 per tier over the three shapes at m = 64, where the window must be more than four binomial
    standard deviations wide on either side.  The emulated draw over those tickets and slots must sit inside it for every m."""
    n, rows_per_wave, waves = 1024, 28, 8
    t, s, w = np.meshgrid(np.arange(n), np.arange(rows_per_wave), np.arange(waves), indexing="ij")
    slot_index = (w * rows_per_wave + s).ravel()  # kb_u + sl: the row's index in the example
    t, w = t.ravel(), w.ravel()
    hot = (slot_index + t * 7) % 3 == 0
    for tier, m in enumerate((8, 16, 32, 64)):
        sel = hot & ((slot_index // 3 + t) % 4 == tier)
        turns = draw_turns(t[sel], slot_index[sel], w[sel], m)
        units, share = int(sel.sum()), float(turns.mean())
        sd = np.sqrt((1 / m) * (1 - 1 / m) / units)
        print(f"m = {m}: {units} units, share {share:.5f} = {share * m:.3f} / m; window +-0.3 / m = {0.3 / m / sd:.1f} binomial sd")
        assert 0.3 / m > 4 * sd
        assert 0.7 / m <= share <= 1.3 / m
