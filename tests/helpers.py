"""Shared helpers for the parity tests: build matching oracle / GPU models and synthetic streams."""
import numpy as np

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
from oracle import fwo

LOGLOSS_TOL = 1e-4   # north_star: per-example log-loss tolerance


def mi_from_cfg(d, wiring="regressor", n_fields=None):
    """ModelInstance from a golden-scenario config dict."""
    F = d.get("ffm_num_fields", 0) if n_fields is None else n_fields
    nc = d.get("num_combos", 1)
    mi = fw.ModelInstance(
        learning_rate=d["learning_rate"], ffm_learning_rate=d["ffm_learning_rate"], bit_precision=d["bit_precision"],
        power_t=d["power_t"], ffm_power_t=d["ffm_power_t"], add_constant_feature=True,
        feature_combo_descs=[fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(nc - 1)],
        ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(F)], ffm_k=d.get("ffm_k", 0),
        ffm_bit_precision=d.get("ffm_bit_precision", 18), ffm_init_acc_gradient=d.get("ffm_init_acc_gradient", 0.0),
        init_acc_gradient=d["init_acc_gradient"], optimizer=d["optimizer"],
        wiring=fw.capi.WIRING_FFM_ONLY if wiring == "ffm_only" else fw.capi.WIRING_REGRESSOR)
    return mi


def make_pair(n_ns, k, bits, ffm_bits, optimizer, lr=0.1, ffm_lr=0.1, power_t=0.5, ffm_power_t=0.5, init_acc=1.0,
              ffm_init_acc=None, interactions=()):
    """(ModelInstance, fw translator, oracle config, oracle translator) for n_ns namespaces == fields, LR --keep for
    every namespace (+ the given namespace-pair interactions) + constant.

    ffm_init_acc defaults to init_acc, as the reference's command line does (model_instance.rs:423:
    ffm_init_acc_gradient defaults to init_acc_gradient).  NOTE: ffm_init_acc=0 with AdaGrad makes every first
    step on a weight +-learning_rate whatever the gradient size; with lr=0.1 on ~10^4 weights per example the
    training dynamics are chaotic and f32 summation-order noise is amplified to O(1) within tens of examples, for
    ANY two implementations that do not add in the same order (the reference's own SSE and scalar paths included).
    Stream-parity tests therefore run in the default regime; the exactness of each mechanism at
    ffm_init_acc=0 is pinned by the KAT scenarios and the crafted single-example cases."""
    if ffm_init_acc is None:
        ffm_init_acc = init_acc
    combos = [fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(n_ns)]
    combos += [fw.FeatureComboDesc([fw.NamespaceDescriptor(a), fw.NamespaceDescriptor(b)]) for a, b in interactions]
    mi = fw.ModelInstance(learning_rate=lr, ffm_learning_rate=ffm_lr, bit_precision=bits, power_t=power_t,
                          ffm_power_t=ffm_power_t, add_constant_feature=True, feature_combo_descs=combos,
                          ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(n_ns)] if k else [], ffm_k=k,
                          ffm_bit_precision=ffm_bits, init_acc_gradient=init_acc, ffm_init_acc_gradient=ffm_init_acc,
                          optimizer=optimizer)
    ocfg = fwo.make_config(optimizer=optimizer, learning_rate=lr, power_t=power_t, init_acc_gradient=init_acc,
                           bit_precision=bits, num_combos=mi.num_combos, ffm_k=k, ffm_bit_precision=ffm_bits,
                           ffm_num_fields=n_ns if k else 0, ffm_learning_rate=ffm_lr, ffm_power_t=ffm_power_t,
                           ffm_init_acc_gradient=ffm_init_acc)
    ots = fwo.TranslatorSpec([([(i, False)], 1.0) for i in range(n_ns)] + [([(a, False), (b, False)], 1.0) for a, b in interactions],
                             [[(i, False)] for i in range(n_ns)] if k else [], True, bits, k, ffm_bits)
    return mi, ocfg, ots


def logloss(p, y):
    """benchmark/calc_loss.py:5-25"""
    p = np.clip(np.asarray(p, dtype=np.float64), 1e-15, 1 - 1e-15)
    y = np.asarray(y)
    return -np.where(y == 1, np.log(p), np.log(1 - p))


def record_labels(records, rec_off):
    return np.array([records[int(o) + 1] for o in rec_off[:-1]], dtype=np.float32)


# ------------------------------------------------------------------ streams: sequential mode == reference single thread
def _stream_parity(n_ns, k, bits, ffm_bits, optimizer, n, mean_extra, p_weighted, ids, seed, interactions=(),
                   weight_tol=2e-5, whole_lines=None, lds_keep=None, kept_rows=None, launches=None, **kw):
    """(`launches`: a list that receives Regressor.last_launch() of the entries' and of the records' launch)"""
    mi, ocfg, ots = make_pair(n_ns, k, bits, ffm_bits, optimizer, interactions=interactions, **kw)
    recs, off = fw.synth_records(n_ns, mean_extra, 1.1, ids, p_weighted, seed, 0, n)
    y = record_labels(recs, off)
    om = fwo.Model(ocfg)
    _, p_ref = om.run_stream(ots, recs, off, holdout_after=0, nthreads=1)
    results = []
    # both ways of feeding the device: entries translated on the host, and raw records translated inside the kernel
    for kind in ("entries", "records"):
        re = fw.Regressor(mi)
        if whole_lines is not None:
            re.set_whole_line_updates(whole_lines)
        if lds_keep is not None:
            re.set_lds_keep(lds_keep)
        if kept_rows is not None:
            re.set_kept_rows(kept_rows)
        fbt = fw.FeatureBufferTranslator(mi)
        b = re.batch_from_records(fbt, recs, off) if kind == "entries" else re.record_batch(fbt, recs, off)
        re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
        if launches is not None:
            launches.append(re.last_launch())
        p_gpu = b.predictions()
        d_ll = np.abs(logloss(p_gpu, y) - logloss(p_ref, y))
        assert d_ll.max() < LOGLOSS_TOL, f"{kind}: max per-example |d logloss| = {d_ll.max()} at {d_ll.argmax()}"
        assert np.abs(p_gpu - p_ref).max() < 5e-5
        # final tables: same state as the reference after the whole stream
        # (weights are O(0.1); accumulators grow to O(100), hence the relative term)
        def close(a, b_):
            return bool(np.all(np.abs(a - b_) <= weight_tol + 1e-5 * np.abs(b_)))

        assert close(re.table_read(capi.TABLE_LR), om.lr_table)
        if k:
            assert close(re.table_read(capi.TABLE_FFM_W), om.ffm_weights)
            acc_g, acc_o = re.table_read(capi.TABLE_FFM_ACC), om.ffm_acc
            assert close(acc_g, acc_o)
            # exactly the same set of accumulators was touched
            a0 = np.float32(mi.ffm_init_acc_gradient if optimizer == fw.Optimizer.AdagradFlex else 0.0)
            assert np.array_equal(acc_g != a0, acc_o != a0)
        results.append((p_gpu, [re.table_checksum(t) for t in (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC)]))
        b.close()
        re.close()
    # device-side translation == host translation, bit for bit (hash indices and everything downstream)
    assert np.array_equal(results[0][0], results[1][0]) and results[0][1] == results[1][1]
    return results[0][0], p_ref


# ------------------------------------------------------------------ streams whose examples share nothing
class DisjointStream:
    """What disjoint_stream returns: raw records (`recs`, `off`), the entry route's FeatureBuffers (`fbs`, the host translator's output, equal
    to the generator's own bookkeeping), and that bookkeeping -- per FEATURE OCCURRENCE, in buffer order: `ex` (example), `hash` (the FFM row's
    first float == the LR index), `fld` (field, -1 for an LR-only namespace), `val`; per ROW (distinct feature): `row_hash`, `row_ex`,
    `row_count` (occurrences in its example) and `row_ffm` (False: an LR-only feature, which has no FFM row)."""


def disjoint_stream(F, k, n, per_field=(1, 1), p_weighted=0.0, p_dup=0.0, seed=0, lr_only_ns=0, first_ffm=None, first_lr=None, scatter=1):
    """n examples over F namespaces (== FFM fields; k = 0: LR only) that share NO FFM row, no 128-byte line of a row and no LR entry, so the
    order in which they are learned cannot matter.  Per field `per_field` = (lo, hi) features (seeded numpy draw), a share `p_weighted` of them
    with a value other than 1, a share `p_dup` followed by the same feature once more in the same field (a chained duplicate row); labels
    0 / 1, importances 1.0 / 0.5.  `lr_only_ns` further namespaces (one feature each) feed the LR block alone.  `first_ffm` / `first_lr`:
    example 0 is padded to exactly that many FFM features (in field 0) / LR entries (in the first LR-only namespace) -- the batch's maxima.

    Row i of the whole batch starts at float i * S + 8 * (i % 4) * (k % 4 == 0), S a multiple of 32 floats >= R + 64: every 32-byte start
    phase of a line occurs (where the translator's mask -- multiples of next_pow2(k) -- allows it) and rows of different examples are a line
    apart.  The raw hash IS that float index: with LR bits >= FFM bits and no interaction combos the LR indices differ like the rows.
    The models must be built with add_constant_feature = False (disjoint_models): the constant's entry would be shared by every example.
    check_disjoint() asserts all of this on the host translator's output.

    `scatter` = m > 1 (a power of two): the 2^ffm_bits table is cut into m equal regions and row i goes into region i % m, (i // m) * S floats into
    it (the phase 8 * (i % 4) as above), so an example's consecutive rows lie in different regions -- with owners taken from a hash's high bits
    (multi-rank modes) at different owners -- and no row crosses a region's end.  The features are drawn first and the slots assigned afterwards:
    values, labels, importances and duplicates are those of the scatter = 1 stream of the same seed.  `span` is then the whole table."""
    rng = np.random.default_rng(seed)
    R = F * k
    S = ((R + 64 + 31) // 32) * 32 if k else 1
    n_ns = F + lr_only_ns
    assert scatter >= 1 and scatter & (scatter - 1) == 0
    row_ex, row_count, row_ffm = [], [], []
    vals = np.array([0.5, 2.0, 0.75, 1.5], dtype=np.float32)
    drawn = []  # per example: (slots[ns] = [(row, value)], label, importance word)
    for e in range(n):
        slots = [[] for _ in range(n_ns)]

        def feature(ns, allow_dup=True):
            i = len(row_ex)
            c = 0
            for _ in range(2 if allow_dup and rng.random() < p_dup else 1):
                v = float(vals[rng.integers(0, 4)]) if rng.random() < p_weighted else 1.0
                slots[ns].append((i, v))
                c += 1
            row_ex.append(e), row_count.append(c), row_ffm.append(bool(k) and ns < F)

        for ns in range(n_ns):
            for _ in range(int(rng.integers(per_field[0], per_field[1] + 1)) if ns < F else 1):
                feature(ns)
        if e == 0 and first_ffm is not None:
            while sum(len(s) for s in slots[:F]) < first_ffm:
                feature(0, allow_dup=False)
            assert sum(len(s) for s in slots[:F]) == first_ffm
        if e == 0 and first_lr is not None:
            while sum(len(s) for s in slots) < first_lr:
                feature(F, allow_dup=False)
            assert sum(len(s) for s in slots) == first_lr
        drawn.append((slots, int(rng.integers(0, 2)), int(np.float32(1.0 if rng.random() < 0.7 else 0.5).view(np.uint32))))
    # the slots: row i of the batch -> its first float
    n_rows = len(row_ex)
    per_region = (n_rows + scatter - 1) // scatter  # rows a region holds
    span = n_rows * S if scatter == 1 else scatter * per_region * S
    ffm_bits = max(10, int(np.ceil(np.log2(span))))  # the smallest table that holds the rows
    assert ffm_bits <= 27, "drop n rather than exceed a 27-bit table"
    region = (1 << ffm_bits) // scatter
    assert per_region * S <= region
    phase = 8 * (np.arange(n_rows) % 4) if k and k % 4 == 0 else 0
    row_hash = ((np.arange(n_rows) % scatter) * region + (np.arange(n_rows) // scatter) * S + phase).astype(np.int64)
    if scatter > 1:
        assert not k or np.all(row_hash % region + R + 32 <= region), "a row (rounded to lines) crosses its region's end"
        span = 1 << ffm_bits
    ex, hsh, fld, val = [], [], [], []
    recs, off = [], [0]
    for e, (slots, label, imp) in enumerate(drawn):
        rec = [0, label, imp] + [0] * n_ns
        for ns, s in enumerate(slots):
            s = [(int(row_hash[i]), v) for i, v in s]
            for h, v in s:
                ex.append(e), hsh.append(h), fld.append(ns if ns < F and k else -1), val.append(v)
            if len(s) == 1 and s[0][1] == 1.0:
                rec[3 + ns] = s[0][0]  # parser.rs:57-74: a single feature of value 1 is its hash
            else:
                start = len(rec)
                for h, v in s:
                    rec += [h, int(np.float32(v).view(np.uint32))]
                assert start <= 0x3fff and len(rec) <= 0xffff
                rec[3 + ns] = 0x80000000 | (start << 16) | len(rec)
        rec[0] = len(rec)
        recs += rec
        off.append(len(recs))
    st = DisjointStream()
    st.F, st.k, st.n, st.R, st.S, st.n_ns, st.lr_only_ns, st.scatter = F, k, n, R, S, n_ns, lr_only_ns, scatter
    st.recs, st.off = np.array(recs, dtype=np.uint32), np.array(off, dtype=np.uint64)
    st.ex, st.hash, st.fld, st.val = np.array(ex), np.array(hsh, dtype=np.int64), np.array(fld), np.array(val, dtype=np.float32)
    st.row_hash, st.row_ex = row_hash, np.array(row_ex)
    st.row_count, st.row_ffm = np.array(row_count), np.array(row_ffm, dtype=bool)
    st.ffm_bits = ffm_bits
    st.bits = st.ffm_bits  # LR bits >= FFM bits: the LR index of a feature is its row's first float
    st.span = span  # floats of the FFM tables (LR entries) that the batch can touch: row i lies inside [i * S, (i + 1) * S) (scatter > 1: the table)
    st.labels = record_labels(st.recs, st.off)
    st.fbs = None
    return st


def disjoint_models(st, optimizer, lr=0.1, ffm_lr=0.1, power_t=0.5, ffm_power_t=0.5, init_acc=1.0, ffm_init_acc=None):
    """(ModelInstance, oracle config, oracle translator) for a disjoint_stream: one LR combo per namespace, one FFM field per namespace of
    the first F, NO constant feature (translate.cpp translate_record: its LR entry would be the one thing every example shares)."""
    ffm_init_acc = init_acc if ffm_init_acc is None else ffm_init_acc
    F, k = st.F, st.k
    mi = fw.ModelInstance(learning_rate=lr, ffm_learning_rate=ffm_lr, bit_precision=st.bits, power_t=power_t, ffm_power_t=ffm_power_t,
                          add_constant_feature=False, feature_combo_descs=[fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(st.n_ns)],
                          ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(F)] if k else [], ffm_k=k, ffm_bit_precision=st.ffm_bits,
                          init_acc_gradient=init_acc, ffm_init_acc_gradient=ffm_init_acc, optimizer=optimizer)
    ocfg = fwo.make_config(optimizer=optimizer, learning_rate=lr, power_t=power_t, init_acc_gradient=init_acc, bit_precision=st.bits,
                           num_combos=mi.num_combos, ffm_k=k, ffm_bit_precision=st.ffm_bits, ffm_num_fields=F if k else 0,
                           ffm_learning_rate=ffm_lr, ffm_power_t=ffm_power_t, ffm_init_acc_gradient=ffm_init_acc)
    ots = fwo.TranslatorSpec([([(i, False)], 1.0) for i in range(st.n_ns)], [[(i, False)] for i in range(F)] if k else [], False, st.bits, k, st.ffm_bits)
    return mi, ocfg, ots


def check_disjoint(st, mi):
    """The condition the whole argument rests on, on the HOST TRANSLATOR's output (fbt.translate): the line-rounded intervals [h, h + R) of
    different examples' FFM rows are pairwise disjoint (asserted on each example's envelope: an example's rows are neighbours in the table;
    scatter > 1: on every row's own interval, sorted and compared with its neighbour -- a row that two examples hold is two equal intervals),
    no LR hash occurs in two examples, and the translator's entries are the generator's own bookkeeping.  Fills st.fbs (the entry route)."""
    fbt = fw.FeatureBufferTranslator(mi)
    assert not mi.add_constant_feature
    fbs, lo, hi, lr_sets = [], [], [], []
    pos = 0
    for e in range(st.n):
        fb = fbt.translate(st.recs[int(st.off[e]):int(st.off[e + 1])], e)
        fbs.append(fb)
        m = len(fb.lr_buffer)
        want_h, want_f, want_v = st.hash[pos:pos + m], st.fld[pos:pos + m], st.val[pos:pos + m]
        assert np.array_equal(fb.lr_buffer["hash"], want_h) and np.array_equal(fb.lr_buffer["value"], want_v), e
        assert fb.label == st.labels[e]
        if st.k:
            sel = want_f >= 0
            h = fb.ffm_buffer["hash"].astype(np.int64)
            # (k = 16: the mask rounds a start 8 or 24 floats into a line down to 0 or 16 -- two of the four phases exist there)
            assert np.array_equal(h, want_h[sel] & int(fbt.ffm_hash_mask)) and np.array_equal(fb.ffm_buffer["value"], want_v[sel]), e
            assert np.array_equal(fb.ffm_buffer["contra_field_index"], want_f[sel] * st.k), e
            assert h.max() + st.R <= (1 << st.ffm_bits) + st.R
            if getattr(st, "scatter", 1) > 1:  # an example's rows lie all over the table: every distinct row's own interval
                u = np.unique(h)
                lo.extend((u * 4) // 128)
                hi.extend(((u + st.R) * 4 - 1) // 128)
            else:
                lo.append((h.min() * 4) // 128)
                hi.append(((h.max() + st.R) * 4 - 1) // 128)
        lr_sets.append(np.unique(fb.lr_buffer["hash"]))
        pos += m
    assert pos == len(st.hash)
    if st.k:
        lo, hi = np.array(lo), np.array(hi)
        order = np.argsort(lo)
        assert np.all(lo[order][1:] > hi[order][:-1]), "two examples' FFM rows touch one 128-byte line"
    allh = np.concatenate(lr_sets)
    assert len(np.unique(allh)) == len(allh), "an LR entry occurs in two examples"
    st.fbs = fbs
    return fbs

