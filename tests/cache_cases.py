"""Request sets for the context-cached predict launches: one context and 24 requests per model shape, drawn so that every branch of the cached route
is taken by construction and not by luck.  Pure numpy: nothing here touches the device (models() alone imports the package).

THE MODEL (models()).  F fields.  Namespace i < F feeds field i; Fs = min(F, 4) further namespaces F + j feed field j as its SECOND namespace, so a
record batch can hold cached and gathered features in one field (a record batch leaves a covered namespace's slot alone, the second namespace is
another slot).  One LR combo per namespace, no constant feature.

HASHES are multiples of next_pow2(k) below 2^ffm_bits (what the translator's mask leaves), the LR index equal to the row start (LR bits == FFM bits)
as in helpers.disjoint_stream; ffm_bits the smallest table that holds N_ROWS = 256 such rows.  Rows overlap and repeat: nothing is written.
VALUES are disjoint_stream's: 1.0, or one of 0.5, 2.0, 0.75, 1.5 with share 0.3.

THE CONTEXT holds c[f] in {0, 1, 2} features of field f, all in the field's own namespace f.  Fields 0..3 are forced to c = 1, 2, 0, 2, the others are
drawn.  Of the fields with c = 2 every fourth (the first, field 1, among them) holds the SAME feature twice: a context holds every occurrence of its
features.

THE REQUESTS add n[f] in {0, 1, 2} features of the candidate's own to field f.
    request 0      gathers nothing: the context alone (an empty FFM buffer after the filter)
    request 1      has no LR entry outside the context's: its own features reuse the rows (hence the LR indices) of context features of OTHER fields
    requests 0-15  candidates for the record route: a field f < Fs gets the candidate's features through its second namespace F + f, a field f >= Fs
                   through its own namespace, and only where the context left that namespace alone (c = 0)
    requests 16-23 add features to the field's own namespace whether the context fills it or not: the merged record's slot is no longer the context's, a
                   record batch must refuse them (fwgpu_block_cache_record_ok) and only the entry route serves them
    forced         n of fields 0, 1, 2 (c = 1, 2, 0) is (r + f) % 3 in request r >= 2, so requests 2-15 and requests 16-23 each show all nine (c, n)
                   classes of the diagonal rule, and in 16-23 field 0 or 1 always adds to a covered namespace; every field with c = 0 gets a feature
                   in some request, so every column of the cached sums meets a non-zero partner
    never          a feature of the candidate's own with the row AND field of a cached one (the filter would drop it: block_ffm.rs:548, 600)

BUFFERS are in the translator's order (feature_buffer.rs:194-335): LR entries namespace by namespace, FFM entries field by field, within a field its
own namespace before its second one, within a namespace the context's features before the candidate's -- the context first.  RECORDS are written like
disjoint_stream's (a single feature of value 1 is its hash in the slot, anything else a range of {hash, value bits} pairs), except that an absent
namespace's slot word is exactly NO_FEATURES = 0x80000000: fwgpu_block_cache_cover_record takes every other word for a filled slot.  The merged
record is the context's record with the candidate's slots rewritten and their pairs appended, as next_vowpal_with_cache leaves it (parser.rs:195-211).

emulate_cached() is the cached route in float32 numpy, with four planted faults; tests/test_cache_cases_cpu.py holds it to ffm_ref.judge_prediction."""
import numpy as np

LR_ENTRY = np.dtype([("hash", "<u4"), ("value", "<f4"), ("combo_index", "<u4")])          # (fwumious_wabbit_amd._capi's, restated: no import of the package)
FFM_ENTRY = np.dtype([("hash", "<u4"), ("value", "<f4"), ("contra_field_index", "<u4")])
NO_FEATURES = 0x80000000  # parser.rs:19
N_REQUESTS, N_RECORD_ROUTE, N_ROWS = 24, 16, 256
REFILL_REQUEST = 17  # the request whose features make the larger context of the refill case
VALUES = np.array([0.5, 2.0, 0.75, 1.5], dtype=np.float32)
P_WEIGHTED = 0.3
FORCED_C = (1, 2, 0, 2)
FAULTS = ("dcf", "count", "chunk", "empty")
# (F, k) -> what is added to the set's seed until the float64 predictions spread (test_cache_cases_cpu.py: std > 0.05, all inside [0.02, 0.98])
SEED_BUMP = {}

# (F, k, kernel family, chunks per row) of tests/test_gpu_cached_predict.py: the smallest shapes at which each branch of the cached launches is taken
CACHED_MATRIX = [(30, 3, "scalar", 2), (30, 10, "scalar", 5), (65, 2, "scalar", 3),     # chunks of 64 floats: two, five (an odd tail), three; 65 + 4 namespaces = three cover words
                 (6, 4, "resident", 1), (30, 8, "resident", 1),                          # chunks of 256 floats from here on
                 (20, 12, "resident", 1), (21, 12, "resident", 1),                       # k no power of two: e0 / k a real division; 252 floats: a partly filled last lane
                 (16, 32, "resident", 2), (5, 64, "resident", 2), (30, 16, "resident", 2),  # two chunks: full, nearly empty (320 floats), 480 floats
                 (30, 12, "vec4", 2), (40, 16, "vec4", 3), (20, 64, "vec4", 5)]          # the generic 16-byte kernel
CACHED_SHAPES = [(F, k) for F, k, _, _ in CACHED_MATRIX]


def next_pow2(k):
    p = 1
    while p < k:
        p *= 2
    return p


class Request:
    """`n` (features of the candidate's own per field), `record_route`, `slots` (per namespace [(hash, value)], the candidate's own), `lr` / `ffm` (the
    WHOLE request's buffers), `rest` (the FFM entries outside the context: what the filter leaves), `rec` (the merged raw record)"""


class RequestSet:
    """F, k, Fs, n_ns, R, ffm_bits, bits, field_ns (per field its namespaces), c (cached features per field), ctx_slots, ctx_lr, ctx_ffm, ctx_rec,
    empty_rec (the record of a context without features), requests"""


def _entries(rs, slots):
    lr = [(h, v, ns) for ns in range(rs.n_ns) for h, v in slots[ns]]
    ffm = [(h, v, f * rs.k) for f in range(rs.F) for ns in rs.field_ns[f] for h, v in slots[ns]]
    return np.array(lr, dtype=LR_ENTRY).reshape(-1), np.array(ffm, dtype=FFM_ENTRY).reshape(-1)


def _write_slots(rec, slots, which):
    """the namespaces `which` of `slots` into the record (a list of words), pairs appended"""
    for ns in which:
        s = slots[ns]
        if not s:
            rec[3 + ns] = NO_FEATURES
        elif len(s) == 1 and s[0][1] == 1.0:
            rec[3 + ns] = s[0][0]  # parser.rs:57-74: a single feature of value 1 is its hash
        else:
            start = len(rec)
            for h, v in s:
                rec += [h, int(np.float32(v).view(np.uint32))]
            assert start <= 0x3fff and len(rec) <= 0xffff
            rec[3 + ns] = NO_FEATURES | (start << 16) | len(rec)
    rec[0] = len(rec)
    return rec


def request_set(F, k, seed=None):
    assert F >= 4
    rng = np.random.default_rng((4000 + 7 * F + k if seed is None else seed) + SEED_BUMP.get((F, k), 0))
    rs = RequestSet()
    rs.F, rs.k, rs.R, rs.Fs = F, k, F * k, min(F, 4)
    rs.n_ns = F + rs.Fs
    P = next_pow2(k)
    rs.ffm_bits = rs.bits = int(np.log2(N_ROWS * P))
    rs.field_ns = [[f] + ([F + f] if f < rs.Fs else []) for f in range(F)]

    def value():
        return float(VALUES[rng.integers(0, 4)]) if rng.random() < P_WEIGHTED else 1.0

    def row():
        return int(rng.integers(0, N_ROWS)) * P

    # ---- the context
    rs.c = np.array([FORCED_C[f] if f < len(FORCED_C) else int(rng.integers(0, 3)) for f in range(F)])
    rs.ctx_slots = [[] for _ in range(rs.n_ns)]
    twos = 0
    for f in range(F):
        if rs.c[f] == 2 and twos % 4 == 0:
            h = row()
            rs.ctx_slots[f] = [(h, value()), (h, value())]
        else:
            hs = []
            while len(hs) < rs.c[f]:
                h = row()
                if h not in hs:
                    hs.append(h)
            rs.ctx_slots[f] = [(h, value()) for h in hs]
        twos += rs.c[f] == 2
    cached = [set(h for h, _ in rs.ctx_slots[f]) for f in range(F)]
    rs.ctx_lr, rs.ctx_ffm = _entries(rs, rs.ctx_slots)
    head = [0, 0, int(np.float32(1.0).view(np.uint32))] + [NO_FEATURES] * rs.n_ns
    rs.empty_rec = np.array(_write_slots(list(head), rs.ctx_slots, []), dtype=np.uint32)
    ctx_rec = _write_slots(list(head), rs.ctx_slots, range(rs.n_ns))
    rs.ctx_rec = np.array(ctx_rec, dtype=np.uint32)

    # ---- the requests
    rs.requests = []
    for r in range(N_REQUESTS):
        q = Request()
        q.record_route = r < N_RECORD_ROUTE
        n = np.array([0 if r == 0 else int(rng.integers(0, 3)) for _ in range(F)])
        if r >= 2:
            for f in range(3):
                n[f] = (r + f) % 3
            for f in range(3, F):
                if rs.c[f] == 0 and r == 2 + f % (N_RECORD_ROUTE - 2):
                    n[f] = max(n[f], 1)
        if q.record_route:
            n[np.array([f for f in range(rs.Fs, F) if rs.c[f] > 0], dtype=np.int64)] = 0  # a covered namespace is left alone
        q.n = n
        q.slots = [[] for _ in range(rs.n_ns)]
        for f in range(F):
            pool = sorted(set(h for z in range(F) if z != f for h in cached[z]) - cached[f])
            ns = F + f if q.record_route and f < rs.Fs else f
            for _ in range(n[f]):
                while True:
                    h = pool[int(rng.integers(0, len(pool)))] if r == 1 else row()
                    if h not in cached[f]:
                        break
                q.slots[ns].append((h, value()))
        whole = [rs.ctx_slots[ns] + q.slots[ns] for ns in range(rs.n_ns)]
        q.lr, q.ffm = _entries(rs, whole)
        _, q.rest = _entries(rs, q.slots)
        q.rec = np.array(_write_slots(list(ctx_rec), whole, [ns for ns in range(rs.n_ns) if q.slots[ns]]), dtype=np.uint32)
        rs.requests.append(q)
    return rs


def classes(rs, requests=None):
    """the (c, n) classes of the diagonal rule that some field of some request shows"""
    return set((int(rs.c[f]), int(q.n[f])) for q in (rs.requests if requests is None else requests) for f in range(rs.F))


def shifted(rs, shift):
    """the set with every FFM row `shift` floats further on: rows off the 16-byte boundary, as raw entry batches may hold them (the entry route only:
    records pass the translator's mask).  The LR entries stay."""
    import copy

    out = copy.copy(rs)
    out.ctx_ffm = rs.ctx_ffm.copy()
    out.ctx_ffm["hash"] += shift
    out.requests = []
    for q in rs.requests:
        q2 = copy.copy(q)
        q2.ffm, q2.rest = q.ffm.copy(), q.rest.copy()
        q2.ffm["hash"] += shift
        q2.rest["hash"] += shift
        out.requests.append(q2)
    return out


def models(rs, optimizer=None):
    """the ModelInstance of a request set: the twin of helpers.disjoint_models (no oracle: nothing here is compared with it)"""
    import fwumious_wabbit_amd as fw

    nd = fw.NamespaceDescriptor
    return fw.ModelInstance(learning_rate=0.1, ffm_learning_rate=0.1, bit_precision=rs.bits, power_t=0.5, ffm_power_t=0.5, add_constant_feature=False,
                            feature_combo_descs=[fw.FeatureComboDesc([nd(i)]) for i in range(rs.n_ns)],
                            ffm_fields=[[nd(ns) for ns in rs.field_ns[f]] for f in range(rs.F)], ffm_k=rs.k, ffm_bit_precision=rs.ffm_bits,
                            init_acc_gradient=1.0, ffm_init_acc_gradient=1.0, optimizer=fw.Optimizer.AdagradLUT if optimizer is None else optimizer)


def warm_tables(F, k, ffm_bits, bits, seed=5):
    """(ffm_w, ffm_acc, lr_tab) float32, the WHOLE tables (2^ffm_bits + F k floats; 2^bits {w, acc} pairs) at ffm_ref.warm_state's scale rule: weights
    uniform in +-s with s^2 / 3 * sqrt(pairs * k) = 0.45 (0.6 s for F < 8), accumulators from [1, 4], LR weights in +-0.6 / sqrt(namespaces)"""
    rng = np.random.default_rng(seed + 31 * F + k)
    pairs = max(1, F * (F - 1) // 2) * k
    s = np.sqrt(1.35 / np.sqrt(pairs)) * (0.6 if F < 8 else 1.0)
    n = (1 << ffm_bits) + F * k
    w = rng.uniform(-s, s, n).astype(np.float32)
    acc = rng.uniform(1.0, 4.0, n).astype(np.float32)
    lr = np.empty(2 << bits, dtype=np.float32)
    lr[0::2] = rng.uniform(-0.6, 0.6, 1 << bits) / np.sqrt(F + min(F, 4))
    lr[1::2] = rng.uniform(1.0, 4.0, 1 << bits)
    return w, acc, lr


# ------------------------------------------------------------------ the cached route in float32
def _sums(F, k, w, ents, T, dcf, cnt):
    """adds the entries, in buffer order, to the field sums T[f][e0] (e0 = z k + kk: the float of the row that faces field z), to the self-pair
    corrections dcf[f] = sum v^2 |own slot|^2 and to the counts -- every operation rounded to float32"""
    R = F * k
    for h, v, cfi in zip(ents["hash"].tolist(), ents["value"], ents["contra_field_index"].tolist()):
        f = cfi // k
        row = w[h:h + R]
        T[f] = T[f] + row * v
        own = row[f * k:(f + 1) * k]
        dcf[f] = dcf[f] + np.sum(own * own, dtype=np.float32) * v * v
        cnt[f] += 1


def emulate_cached(F, k, w, lr, ctx, cand, fault=None):
    """The prediction of one request in the cached order, float32 throughout.  ctx: the context's FFM entries; cand: (the request's LR entries, the FFM
    entries outside the context).  The context's sums, dcf and counts are formed first (setup_cache); the candidate's features are added to them, a
    field it leaves empty keeps the cache's sums; the diagonal is 0 for c + n <= 1 and 0.5 (|T_ff|^2 - dcf) otherwise.
    fault: None, or one of FAULTS --
        "dcf"    dcf is dropped from the cache (only the candidate's own self pairs are taken out)
        "count"  the count rule uses n alone
        "chunk"  a gathered field reads floats 256.. of its cached row from floats 0.. (where R <= 256: the row's last float reads zero)
        "empty"  a field the candidate leaves empty is filled with zeros instead of the cache's sums"""
    assert fault is None or fault in FAULTS
    w = np.asarray(w, dtype=np.float32)
    lr_ent, rest = cand
    R = F * k
    cT, cdcf, ccnt = np.zeros((F, R), np.float32), np.zeros(F, np.float32), np.zeros(F, np.int64)
    _sums(F, k, w, ctx, cT, cdcf, ccnt)
    gathered = np.zeros(F, dtype=bool)
    gathered[(rest["contra_field_index"] // k).astype(np.int64)] = True
    start = cT.copy()
    if fault == "chunk":
        if R > 256:
            start[gathered, 256:] = cT[gathered, :R - 256]
        else:
            start[gathered, R - 1] = 0.0
    if fault == "empty":
        start[~gathered] = 0.0
    T, dc, n = start, np.zeros(F, np.float32), np.zeros(F, np.int64)
    _sums(F, k, w, rest, T, dc, n)
    dcf = dc if fault == "dcf" else dc + cdcf
    total = n if fault == "count" else n + ccnt
    T3 = T.reshape(F, F, k)
    pair = np.sum(T3 * T3.transpose(1, 0, 2), axis=2, dtype=np.float32)  # pair[f][z] = T[f][z] . T[z][f]
    diag = np.where(total <= 1, np.float32(0.0), np.float32(0.5) * (np.diag(pair) - dcf)).astype(np.float32)
    lr_w = np.asarray(lr, dtype=np.float32)[2 * lr_ent["hash"].astype(np.int64)]
    logit = np.sum(lr_w * lr_ent["value"], dtype=np.float32) + np.sum(pair[np.tril(np.ones((F, F), dtype=bool), -1)], dtype=np.float32) \
        + np.sum(diag, dtype=np.float32)
    if np.isnan(logit):
        return np.float32(0.5)
    logit = np.float32(min(max(logit, np.float32(-50.0)), np.float32(50.0)))
    return np.float32(1.0) / (np.float32(1.0) + np.exp(-logit, dtype=np.float32))
