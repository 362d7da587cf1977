"""ONE step of every route that learns outside the fused single-GPU launch, judged per float against float64 (tests/ffm_ref.py, the same C and C_P).

The routes: the synchronous micro-batch on one GPU (fwgpu_learn_batch_sync: the FWD / MID / UPD phase kernels), the owner-sharded micro-batch
(fwgpu_dist_group_learn_sharded: the same phases with owned ranges, split records summed over the ranks), the peer-sharded step (the fused kernel
with a table base looked up per row), the owner-side apply step by step (the push branch + owner_apply_kernel) and its streaming form (the
streaming push + owner_stream_consume).  Each has gradient or update code of its own, and each was held to stream bars only.

The probes (ffm_ref.dist_probe_stream) share no row, no line and no LR entry, so whatever rank runs an example, whoever owns a row and whenever
the owner applies a gradient, every route must leave what ONE sequential step per example leaves: ffm_ref.judge_example on the device's own
before- and after-state, read from every rank BEFORE any gather and judged in the OWNER's copy of each float.  The rows of an example lie in all
four quarters of the table (scatter = 4): with 2 or 4 ranks at every owner, none across an ownership boundary.  Every float outside the rows a
rank owns is bit-identical on that rank; after gather_tables all ranks hold the owners' ranges put together.  The two routes whose owners apply
concurrently (learn_owner under MODE_HOGWILD, learn_owner_stream) get probes without chained duplicates: two occurrences of one row are pushed
and applied by different waves there and race inside the owner, by design.

What would turn which case red (planted on a float32 model of the owner route in tests/test_ffm_ref_cpu.py): a dropped second 256-float chunk of
a pushed row (5x64, 16x32, 40x16: floats 256.. keep their old value); z by a shift where k is no power of two (20x12, 30x10, 30x3: the self-pair
term lands on another slot's floats); a pushed row applied twice or a slot handed back before its tail was read (every float of the row steps
twice / takes another row's gradient); an accumulator not stored under AdagradFlex (acc keeps its old value).

Which phase kernels a shape takes (launch_example_phase reports nothing through last_launch; from its rule: T moves from LDS into the split
record once twice the staged footprint exceeds 160 KiB): 40x16 holds 4 * 40 * 640 = 102 400 bytes of T alone, more than half of 160 KiB whatever
the batch -- t_global = 1 in FWD and UPD.  30x16 holds 57 600 bytes of T; the rest of the staged footprint at these probes (at most ~70 features:
own slots 4.5 KB, the AdaGrad LUT 8 KB, entry arrays and sets under 4 KB) stays below 24 KB, so its phases stage T in LDS: the largest staged
shape.  Every other shape of the matrix is far below.  k % 4 != 0 (30x3, 30x10) takes the VEC = 1 phases.  The sharded route brings the same number of
probes on every rank (fwgpu_dist_group_learn_sharded requires it); the other routes deal them unevenly.

Measured on the MI355X (the DISTSTEP lines): the micro-batch, sharded, peer and in-order owner routes need at most 0.124 C (20x12, an accumulator of a
chained duplicate) and 0.009 C_P; the concurrent owner route and the streaming form, whose probes have no duplicates, 0.005 C -- on every case the
oracle's own figure for that probe set: no route needs a constant of its own."""
import numpy as np
import pytest

import ffm_ref
import fwumious_wabbit_amd as fw
from ffm_ref import DIST_MATRIX, FLEX, LUT, SGD
from fwumious_wabbit_amd import _capi as capi
from fwumious_wabbit_amd.dist import DistGroup
from helpers import check_disjoint, disjoint_models

pytestmark = pytest.mark.gpu

TABLES = (capi.TABLE_FFM_W, capi.TABLE_FFM_ACC, capi.TABLE_LR)
SEQ, HOG = capi.MODE_SEQUENTIAL, capi.MODE_HOGWILD
OPT_SHAPES = [(6, 4), (30, 10), (40, 16)]   # SGD and AdagradFlex: one shape per family of paths
FOUR_RANK_SHAPES = [(30, 10), (40, 16)]     # the scalar and the three-chunk 16-byte paths at four owners
UNEVEN = {2: (12, 8), 4: (7, 6, 4, 3)}
EVEN = {2: (10, 10), 4: (5, 5, 5, 5)}

_PROBES = {}


def _probe(F, k, dup):
    """(stream, warm state) of the shape, generated and checked once, left unchanged"""
    if (F, k, dup) not in _PROBES:
        st = ffm_ref.dist_probe_stream(F, k, dup)
        mi, _, _ = disjoint_models(st, LUT)
        check_disjoint(st, mi)
        _PROBES[(F, k, dup)] = (st, ffm_ref.warm_state(st))
    return _PROBES[(F, k, dup)]


def _bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _dist_step(route, F, k, opt=LUT, split=None, mode=SEQ, dup=True):
    """the case: `split` = probes per rank (None: one regressor, no group).  Returns the largest needed c / C."""
    st, warm = _probe(F, k, dup)
    mi, ocfg, _ = disjoint_models(st, opt, **ffm_ref.opt_kwargs(opt))
    cfg = ffm_ref.StepConfig.from_oracle_config(ocfg)
    fbs, R = st.fbs, st.R
    N = len(split) if split is not None else 1
    assert sum(split) == st.n if split is not None else True
    lg = N.bit_length() - 1
    assert 1 << lg == N
    regs = [fw.Regressor(mi) for _ in range(N)]
    fbt = fw.FeatureBufferTranslator(mi)
    g = sp = batch = None
    try:
        for re in regs:
            for t, v in zip(TABLES, warm):
                re.table_write(t, v)
        before = [[re.table_read(t) for t in TABLES] for re in regs]
        for j in range(1, N):
            for a, b in zip(before[0], before[j]):
                assert _bits_equal(a, b)
        assert len(before[0][0]) == (1 << st.ffm_bits) + R and len(before[0][2]) == 2 << st.bits  # the warm state covers the whole tables
        # ---- the step
        if split is None:
            batch = regs[0].record_batch(fbt, st.recs, st.off)
            sp = regs[0].split_buffers(st.n, max(len(fb.ffm_buffer) for fb in fbs))
            regs[0].learn_batch_sync(batch, sp, mode)
            p = batch.predictions().copy()
        else:
            g = DistGroup(regs)
            g.set_mode(mode)
            cut = np.concatenate([[0], np.cumsum(split)])
            rr = [st.recs[int(st.off[cut[j]]):int(st.off[cut[j + 1]])] for j in range(N)]
            oo = [st.off[cut[j]:cut[j + 1] + 1] - st.off[cut[j]] for j in range(N)]
            if route == "sharded":
                outs = g.learn_sharded(fbt, rr, oo)
            elif route == "peer":
                outs = g.learn_peer(fbt, rr, oo)
            elif route == "owner":
                outs = g.learn_owner(fbt, rr, oo)
            else:
                outs = g.learn_owner_stream(fbt, rr, oo, log2_rows=6, log2_lr=6)
            p = np.concatenate(outs)
        after = [[re.table_read(t) for t in TABLES] for re in regs]  # (before any gather)
        launches = [re.last_launch() for re in regs]
        gathered = None
        if g is not None:
            g.gather_tables()
            gathered = [[re.table_read(t) for t in TABLES] for re in regs]
    finally:
        if batch is not None:
            batch.close()
        if sp is not None:
            sp.close()
        if g is not None:
            g.close()
        for re in regs:
            re.close()
    assert len(p) == st.n and np.all(np.isfinite(p))
    # ---- the owners' copies put together: rank j owns the FFM rows that start in its 1 / N of 2^ffm_bits (the last rank: with the table's R-float
    # tail) and the LR entries in its 1 / N of 2^bits
    per_f, per_l = (1 << st.ffm_bits) // N, (1 << st.bits) // N
    f_lo = [j * per_f for j in range(N)]
    f_hi = [(j + 1) * per_f for j in range(N - 1)] + [(1 << st.ffm_bits) + R]
    owned = [t.copy() for t in after[0]]
    for j in range(1, N):
        owned[0][f_lo[j]:f_hi[j]] = after[j][0][f_lo[j]:f_hi[j]]
        owned[1][f_lo[j]:f_hi[j]] = after[j][1][f_lo[j]:f_hi[j]]
        owned[2][2 * j * per_l:2 * (j + 1) * per_l] = after[j][2][2 * j * per_l:2 * (j + 1) * per_l]
    # ---- the kernel the step ran on, where the route reports it (the fused kernel with the owner lookup: the generic family)
    if route in ("peer", "owner", "stream"):
        for j in range(N):
            if split[j]:
                want = (capi.KERNEL_SCALAR, (R + 63) // 64) if k % 4 else (capi.KERNEL_VEC4, (R + 255) // 256)
                assert (launches[j]["family"], launches[j]["chunks"]) == want, (j, launches[j])
    # ---- every probe, in the owners' copies
    worst, where, skipped, worst_p = 0.0, None, 0, 0.0
    touched, lr_touched = [], []
    for e, fb in enumerate(fbs):
        v = ffm_ref.judge_example(cfg, before[0], owned, fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, p[e])
        assert v.p_err <= v.p_bound, f"example {e}: prediction {p[e]!r}, float64 {v.ref.p!r}: |d| = {v.p_err:.3e}, bound {v.p_bound:.3e} (needs c_p = {v.p_ratio:.3e}, C_P = {ffm_ref.C_P:.3e})"
        worst_p = max(worst_p, v.p_ratio)
        skipped += v.skipped
        touched.append(v.ref.ffm_idx), lr_touched.append(v.ref.lr_idx)
        if v.worst > worst:
            worst, where = v.worst, (e,) + v.where
    ranks = "-" if split is None else "+".join(str(s) for s in split)
    print(f"DISTSTEP {route}{'' if mode == SEQ else '-concurrent'} {F}x{k} opt={opt} ranks={ranks}: needs c = {worst:.3e} = {worst / ffm_ref.C:.3f} C at {where}, "
          f"c_p = {worst_p:.3e} = {worst_p / ffm_ref.C_P:.3f} C_P, {skipped} probes skipped")
    if where is not None and worst > ffm_ref.C:
        e, name, idx = where
        if name in ("w", "acc"):
            rows = np.unique(fbs[e].ffm_buffer["hash"].astype(np.int64))
            h = int(rows[np.searchsorted(rows, idx, side="right") - 1])
            n_occ = int(np.sum(fbs[e].ffm_buffer["hash"] == h))
            raise AssertionError(f"example {e}, table {name}, float {idx}: row at {h} (owner {h // per_f}, {n_occ} occurrence(s)), float {idx - h} of the row = field slot "
                                 f"{(idx - h) // k}, chunk of 256 {(idx - h) // 256}, chunk of 64 {(idx - h) // 64}: needs c = {worst:.3e}, C = {ffm_ref.C:.3e}")
        raise AssertionError(f"example {e}, table {name}, LR entry {idx} (owner {idx // per_l}): needs c = {worst:.3e}, C = {ffm_ref.C:.3e}")
    assert skipped <= ffm_ref.MAX_SKIPPED_SHARE * st.n
    # ---- no rank wrote anything but the touched floats of the rows and entries it owns
    touched, lr_touched = np.concatenate(touched), np.concatenate(lr_touched)
    for j in range(N):
        mine = touched[(touched >= f_lo[j]) & (touched < f_hi[j])]
        lmine = lr_touched[lr_touched // per_l == j]
        assert ffm_ref.untouched_identical(before[j][0], after[j][0], mine), f"rank {j}, FFM_W: a float outside the rows it owns changed"
        assert ffm_ref.untouched_identical(before[j][1], after[j][1], mine if opt != SGD else np.zeros(0, dtype=np.int64)), f"rank {j}, FFM_ACC: a float outside the rows it owns changed"
        assert ffm_ref.untouched_identical(before[j][2], after[j][2], np.concatenate([2 * lmine, 2 * lmine + 1] if opt != SGD else [2 * lmine])), f"rank {j}, LR: an entry it does not own changed"
    assert not _bits_equal(before[0][0], owned[0]), "the step changed no weight"
    # ---- the scatter layout did what the case needs: every owner holds rows of several examples, an example's rows lie at several owners
    if N > 1:
        for j in range(N):
            n_ex = sum(1 for fb in fbs if np.any(fb.ffm_buffer["hash"].astype(np.int64) // per_f == j))
            assert n_ex >= 3, (j, n_ex)
            assert not _bits_equal(before[j][0], after[j][0]), f"owner {j} stepped nothing"
        for e, fb in enumerate(fbs):
            if len(np.unique(fb.ffm_buffer["hash"])) >= 4:
                assert len(np.unique(fb.ffm_buffer["hash"].astype(np.int64) // per_f)) >= 2, e
    # ---- after the gather every rank holds the owners' ranges put together
    if gathered is not None:
        for j in range(N):
            for a, b in zip(gathered[j], owned):
                assert _bits_equal(a, b), f"rank {j} after gather_tables"
    return worst / ffm_ref.C


def _cases(ranks2=True, four=True, opts=True, split_by=UNEVEN, extra=()):
    """(F, k, opt, split): AdagradLUT on every shape with two ranks (or none), four ranks on two shapes, SGD and AdagradFlex on three shapes"""
    out = [(F, k, LUT, split_by[2] if ranks2 else None) for F, k in DIST_MATRIX]
    if four:
        out += [(F, k, LUT, split_by[4]) for F, k in FOUR_RANK_SHAPES]
    if opts:
        out += [(F, k, o, split_by[2] if ranks2 else None) for F, k in OPT_SHAPES for o in (SGD, FLEX)]
    return out + list(extra)


def _id(c):
    F, k, opt, split = c
    return f"{F}x{k}-{ {LUT: 'lut', SGD: 'sgd', FLEX: 'flex'}[opt] }" + ("" if split is None else "-" + "+".join(str(s) for s in split))


@pytest.mark.parametrize("c", _cases(ranks2=False, four=False), ids=_id)
def test_synchronous_micro_batch_on_one_gpu(c):
    """fwgpu_learn_batch_sync, MODE_SEQUENTIAL: fw_example_kernel<PH = 1>, split_mid_kernel, fw_example_kernel<PH = 3>"""
    F, k, opt, _ = c
    _dist_step("sync", F, k, opt)


@pytest.mark.parametrize("c", _cases(split_by=EVEN), ids=_id)
def test_sharded_micro_batch(c):
    """fwgpu_dist_group_learn_sharded: the phases over owned ranges, the ranks' split records summed in rank order (restates
    test_sharded_ranks_touch_only_their_own_range at these shapes: no rank writes outside the rows it owns)"""
    F, k, opt, split = c
    _dist_step("sharded", F, k, opt, split)


@pytest.mark.parametrize("c", _cases(), ids=_id)
def test_peer_sharded_step_in_order(c):
    """fwgpu_dist_group_learn_peer, MODE_SEQUENTIAL: fw_example_kernel<SH = true>, every row reached in its owner's tables"""
    F, k, opt, split = c
    _dist_step("peer", F, k, opt, split)


@pytest.mark.parametrize("c", _cases(four=False), ids=_id)
def test_peer_sharded_step_concurrent(c):
    """... MODE_HOGWILD: the ranks' kernels at once, the examples of a rank concurrently (chained duplicates stay inside a workgroup)"""
    F, k, opt, split = c
    _dist_step("peer", F, k, opt, split, mode=HOG)


@pytest.mark.parametrize("c", _cases(extra=[(30, 8, LUT, (0, 20))]), ids=_id)
def test_owner_side_apply_in_order(c):
    """fwgpu_dist_group_learn_owner, MODE_SEQUENTIAL: in-order pushes, the in-order single-wave owner_apply_kernel; once with a source that
    brings nothing (0 + 20)"""
    F, k, opt, split = c
    _dist_step("owner", F, k, opt, split)


@pytest.mark.parametrize("c", _cases(), ids=_id)
def test_owner_side_apply_concurrent(c):
    """... MODE_HOGWILD: a wave per pushed row on both sides, the 16-byte and the scalar path of owner_apply_kernel (no chained duplicates:
    they race inside the owner by design)"""
    F, k, opt, split = c
    _dist_step("owner", F, k, opt, split, mode=HOG, dup=False)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_ranks", [1, 2])
@pytest.mark.parametrize("c", _cases(ranks2=False, four=False), ids=_id)
def test_owner_side_apply_streaming(c, n_ranks):
    """fwgpu_dist_group_learn_owner_stream with regions of 64 slots -- fewer than the step's gradient rows and LR words, so slots are reused and
    the flow control runs -- on one and two in-process ranks (four need a process of their own: test_gpu_dist.py).  The library's own deadline
    and abort word end a stuck step; a case that runs into the time limit is a hang, not a flaky test."""
    F, k, opt, _ = c
    _dist_step("stream", F, k, opt, {1: (20,), 2: UNEVEN[2]}[n_ranks], mode=HOG, dup=False)
