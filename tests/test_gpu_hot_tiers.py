"""Store policy 4 thins a hot row's accumulator adds by the row's heat (csrc/hot_tiers.h): one example in 8 up to 8 theta, one in 16 / 32 / 64 beyond
8 / 16 / 32 theta.  Checked per float on streams whose examples share no row (tests/test_gpu_concurrent_exact.py's rig: the in-order launch is the
reference for every float), and as a sum on rows that a third of all examples hold (tests/test_gpu_conservation.py's rig).

What would turn which case red:
  * a tier's level compared against the wrong accumulator, or a slot's tier bits handed to another slot behind the pipelined loop: a unit preset to one
    tier shows another tier's multiple of the in-order delta (m x d within m ulps is asserted with the unit's OWN m);
  * the turn tested with the base mask where the add multiplies by the row's m (or the reverse): the share of turns of that tier is 1/8 where it must
    be 1/m, or the delta is 8 d;
  * re-read rows or the two-chunk kernel's units (update_rows_win) left on the base exponent: the units of c_k16 / c_f40, and the re-read ones of case a,
    show 8 d at presets of 12, 24 and 48 theta;
  * a draw whose higher bits are not uniform over tickets and slots: the share of a tier leaves [0.7 / m, 1.3 / m];
  * option 15 = 0 not restoring the parent's launches: a preset beyond 8 theta shows anything but 8 d.
"""
import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
from helpers import disjoint_models

import test_gpu_concurrent_exact as cx
import test_gpu_conservation as cons

pytestmark = pytest.mark.gpu

LUT, FLEX = fw.Optimizer.AdagradLUT, fw.Optimizer.AdagradFlex
THETA = 0.5  # the default threshold
HEATS = (3 * THETA, 12 * THETA, 24 * THETA, 48 * THETA)  # one preset inside each tier, none on a level
TIER_M = (8, 16, 32, 64)

# Units per tier at m = 64 decide the size: the window 0.7 / m .. 1.3 / m must be more than four binomial standard deviations wide, i.e. more than
# 4^2 (m - 1) / 0.3^2 = 11 200 units of that tier.  Case a has ~19 000 per tier at 1024 examples (~225 rows each, every third hot, a quarter per tier); the
# two-chunk shapes have 2 units per row but only ~60 / ~80 rows per example: c_k16 needs 2048 examples (~20 000 per tier), c_f40 has ~13 500 at 1024.
STREAMS = {
    "a": dict(cx.A_STREAM),
    "c_k16": dict(cx.HOT_STREAMS["c_k16"], n=2048),
    "c_f40": dict(cx.HOT_STREAMS["c_f40"]),
}


class _Tiered:
    """Both launches of one case: hot row j (every third feature) preset to init + HEATS[j % 4] on every float.  Gradients differ per float."""

    def __init__(self, shape, opt, tiers):
        st = self.st = cx._stream(**STREAMS[shape])
        assert st.lr_only_ns == 0 and st.k % 4 == 0
        mi, _, _ = disjoint_models(st, opt, **(dict(init_acc=1.0) if opt == FLEX else {}))
        nrows, S = len(st.row_hash), st.S
        self.start = st.row_hash & int(fw.FeatureBufferTranslator(mi).ffm_hash_mask)
        self.hot = np.arange(nrows) % 3 == 0
        self.tier = (np.arange(nrows) // 3) % 4  # of the hot rows: each tier in turn
        a_init = cx._initial_acc(opt, mi.ffm_init_acc_gradient)
        acc0 = np.full(nrows * S, a_init, dtype=np.float32)
        rows = cx._RowView(acc0, self.start, S, st.R)
        for t, heat in enumerate(HEATS):
            rows[self.hot & (self.tier == t)] = np.float32(a_init + heat)
        base = cx._setup(whole=3 if shape == "a" else 2, policy=4)

        def setup_re(re):
            base(re)
            re.set_hot_row_sampling(tiers=tiers)
            re.table_write(capi.TABLE_FFM_ACC, acc0)

        # predictions, FFM weights and the whole LR table (no LR entry is hot here): bit-equal
        self.re_s, self.re_h, _ = cx._modes_agree(mi, st, setup_re, "records", tables=(capi.TABLE_FFM_W, capi.TABLE_LR), keep=True)
        try:
            n = nrows * S
            self.acc0 = rows.copy()
            self.acc_s, self.acc_h = self.re_s.table_read(capi.TABLE_FFM_ACC, 0, n), self.re_h.table_read(capi.TABLE_FFM_ACC, 0, n)
        finally:
            self.re_s.close(), self.re_h.close()

    def check_cold(self):
        s, h = self.acc_s.view(np.uint32).copy(), self.acc_h.view(np.uint32).copy()
        cx._RowView(s, self.start, self.st.S, self.st.R)[self.hot] = 0
        cx._RowView(h, self.start, self.st.S, self.st.R)[self.hot] = 0
        bad = np.flatnonzero(s != h)
        assert not len(bad), f"{len(bad)} accumulators outside the hot rows differ, first at table float {int(bad[0])}"

    def shares(self, m_of_tier):
        """per tier: (units, share whose turn came); asserts that every live unit shows nothing or its tier's m times the in-order delta within m ulps"""
        st = self.st
        rv = lambda t: cx._RowView(t, self.start, st.S, st.R)[self.hot].astype(np.float64)
        a0, s, h = self.acc0[self.hot].astype(np.float64), rv(self.acc_s), rv(self.acc_h)
        tier = self.tier[self.hot]
        d, r = s - a0, h - a0
        # (not every row grows in order: at a preset of 24 a g^2 below half an ulp, 9.5e-7, adds nothing; a unit on which the in-order launch added nothing says nothing)
        assert np.mean((d > 0).any(axis=1)) > 0.9, "the in-order launch must have grown the hot rows"
        if st.R > 256:  # two 1 KiB chunks counted from the row's first line (whole-line launch), as in test_hot_rows_default_sampling
            first = np.arange(st.R)[None, :] < 256 - (self.start[self.hot] % 32)[:, None]
            units = [first, ~first]
        else:
            units = [np.ones_like(d, dtype=bool)]
        out = []
        for t, m in enumerate(m_of_tier):
            sel = tier == t
            zero, full = r[sel] == 0.0, np.abs(r[sel] - m * d[sel]) <= m * cx._ulps(s[sel])
            half = np.abs(r[sel] - 0.5 * m * d[sel]) <= 0.5 * m * cx._ulps(s[sel])  # (would the next lower m fit the unit too?  Then the unit cannot tell them apart)
            n_units = n_turn = n_amb = 0
            for u in units:
                u = np.broadcast_to(u, d.shape)[sel]
                live = ((d[sel] > 0) & u).any(axis=1)
                z, f = (zero | ~u).all(axis=1), (full | ~u).all(axis=1)
                bad = np.flatnonzero(live & ~(z | f))
                assert not len(bad), (f"tier {t} (preset {HEATS[t] / THETA:g} theta, m = {m}): {len(bad)} of {int(live.sum())} hot units are neither untouched nor m x the in-order delta; "
                                      f"first: floats that are 0: {int((zero & u)[bad[0]].sum())}, m d: {int((full & u)[bad[0]].sum())} of {int(u[bad[0]].sum())}; "
                                      f"delta / in-order delta there: {np.unique(np.round(r[sel][bad[0]][u[bad[0]]] / np.maximum(d[sel][bad[0]][u[bad[0]]], 1e-30), 1))[:6]}")
                n_units += int(live.sum())
                n_turn += int((live & f & ~z).sum())
                n_amb += int((live & f & ~z & (half | ~u).all(axis=1)).sum())
            assert n_amb <= 0.5 * n_turn, f"tier {t}: {n_amb} of the {n_turn} units whose turn came would pass as m = {m // 2} too: the gradients are too small to tell"
            out.append((n_units, n_turn / max(n_units, 1)))
        return out


@pytest.mark.parametrize("shape,opt", [("a", LUT), ("a", FLEX), ("c_k16", LUT), ("c_f40", LUT)], ids=["a-lut", "a-flex", "c_k16-lut", "c_f40-lut"])
def test_hot_rows_are_thinned_by_their_tier(shape, opt):
    """Tiers on: a concurrent launch leaves predictions, weights, LR table and every cold accumulator bit-equal to the in-order launch; a hot unit shows nothing or
    m x the in-order delta within m ulps (d's own rounding scaled by m, plus the add's), m = 8 / 16 / 32 / 64 for presets of 3 / 12 / 24 / 48 theta above the
    initial value (0 for AdagradLUT, 1.0 for AdagradFlex); the turn came for a share of each tier's units between 0.7 / m and 1.3 / m -- a condition, more than four
    binomial standard deviations wide at these sizes (asserted), which an ideal draw meets (tests/test_hot_tiers_cpu.py)."""
    hr = _Tiered(shape, opt, tiers=1)
    hr.check_cold()
    res = hr.shares(TIER_M)
    print()
    for (units, share), m in zip(res, TIER_M):
        sd = np.sqrt((1.0 / m) * (1.0 - 1.0 / m) / max(units, 1))
        print(f"{shape} m = {m}: {units} hot units, turn came for {share:.5f} = {share * m:.3f} / m (window: +-{0.3 / m / sd:.1f} binomial sd)")
    assert sum(u for u, _ in res) >= 20000
    for (units, share), m in zip(res, TIER_M):
        assert 0.3 / m > 4.0 * np.sqrt((1.0 / m) * (1.0 - 1.0 / m) / units), (m, units)
        assert 0.7 / m <= share <= 1.3 / m, (m, units, share)


@pytest.mark.parametrize("shape", ["a", "c_k16"])
def test_tiers_off_is_one_example_in_eight_at_every_heat(shape):
    """fwgpu_debug_set_option(h, 15, 0): the four presets all show m = 8, as before the tiers."""
    hr = _Tiered(shape, LUT, tiers=0)
    hr.check_cold()
    res = hr.shares((8, 8, 8, 8))
    print()
    for (units, share), heat in zip(res, HEATS):
        print(f"{shape} preset {heat / THETA:g} theta, tiers off: {units} hot units, turn came for {share:.5f} = {share * 8:.3f} / 8")
        assert 0.7 / 8 <= share <= 1.3 / 8, (heat, units, share)


# ------------------------------------------------------------------ conservation: the sum of g^2 that reaches a row hotter than the first level
CONS_N = 16384


@pytest.mark.parametrize("ffm_bits", [18, 28])
def test_thinned_adds_of_every_tier_count_every_gradient(ffm_bits, capsys):
    """test_gpu_conservation.py's rig (a row in a third of all examples, the same gradient on every float), rows starting at heat 12, 24 and 48 theta: one example
    in 16 / 32 / 64 adds 16 / 32 / 64 times its g^2, and the share of the true sum of g^2 that reaches the accumulators stays around 1.  Tolerance: that test's
    0.1 for one in eight, times sqrt(m / 8) -- the sampling error grows with the root of the thinning.
    One launch size, n = 16 384 (~5 460 hits per row, ~85 turns at m = 64), meets it; 65 536 is not needed.  The draw emulated on the CPU over this rig's tickets
    (the hits of each of the three rows, both slot positions) gives a mean share of turns x m of 1.000 / 1.000 / 1.000 / 0.992-1.000 for m = 8 / 16 / 32 / 64
    (single rows 0.90-1.13 at m = 64).  The rows grow by ~0.25 in such a launch, so none crosses a level."""
    rig = cons.Rig(LUT, ffm_bits)
    rig.re.set_hot_row_sampling(tiers=1)
    table = {}
    try:
        for heat, m in zip(HEATS[1:], TIER_M[1:]):
            for hot_field in (0, 29):
                for key, kw in ((4, {}), ("4 L0", dict(lds_keep=0))):
                    table[(m, hot_field, key)] = float(np.mean([f[0] for f in rig.run(CONS_N, hot_field, 4, 0, acc_start=heat, **kw)]))
    finally:
        rig.close()
    with capsys.disabled():
        print(f"\nshare of the true sum of g^2 that reaches a hot row's accumulators by tier, adagrad, {ffm_bits}-bit table, {CONS_N}-example launches")
        print("  start (theta)  m   hot_field  policy 4  policy 4, nothing parked in LDS   tolerance")
        for heat, m in zip(HEATS[1:], TIER_M[1:]):
            for hot_field in (0, 29):
                print(f"  {heat / THETA:13g} {m:3d}  {hot_field:9d} {table[(m, hot_field, 4)]:9.4f} {table[(m, hot_field, '4 L0')]:9.4f}   {0.1 * np.sqrt(m / 8.0):27.3f}")
    for (m, hot_field, key), share in table.items():
        assert abs(share - 1.0) <= 0.1 * np.sqrt(m / 8.0), (m, hot_field, key, share)
