"""One learning step of the LR + FFM model in float64, and the judge that compares a float32 implementation with it.

A numpy restatement of ONE example's step by the oracle's rules (oracle/fw_oracle.c: lr_forward / ffm_fb_forward / sigmoid_block / ffm_fb_update /
lr_update, the optimizers), every sum and product in float64.  It is to the example kernels what head_ref.py is to the deep head: the plain,
high-precision statement that both the oracle and the device are judged against.

    forward    T[f][z] = sum over the features i of field f of v_i * w_i[z]        (w_i[z]: the k floats of row i that face field z)
               FFM term = sum_{f > z} T[f][z] . T[z][f] + 1/2 sum_f (T[f][f] . T[f][f] - sum_{i in f} v_i^2 w_i[f] . w_i[f])   (the self pair taken out)
               logit = LR sum + FFM term; NaN -> p = 1/2, g = 0; beyond +-50 -> p = logistic(+-50), g = 0; else g = (p - y) * importance
    gradients  per occurrence i (field f) and float (z, kk): grad = g * v_i * (T[z][f] - [z == f] * w_i * v_i) -- w ALWAYS the pre-update weight,
               for the second occurrence of a chained duplicate row too (the oracle caches the gradients before it steps anything)
    steps      SGD: w -= grad * lr.   AdagradFlex: acc += grad^2; w -= grad * lr * acc^-power_t.   AdagradLUT: acc += grad^2; w -= grad * lut[key(acc)],
               lut the ORACLE's own table and key taken from the FLOAT32 new accumulator the caller passes in (`acc_after`: the judged implementation's
               own), so a sum that lands next to a bucket boundary needs no exception.  The occurrences of one row are applied in buffer order on a
               running copy (for the first of two occurrences the float32 key comes from the running float64 sum: the judged state does not hold it).
    outputs    per touched float dw, dacc and the magnitude M = lr * |g| * |v| * sum_i |v_i| |w_i| (the sum behind T[z][f]), summed over the row's
               occurrences, and A = sum 2 |grad| M / lr for the accumulator; the same for LR entries (M = lr * |g| * |v|).

THE JUDGE (judge_floats):  |after - (before + d)| <= c * M + ulp(before) / 2 + ulp(after) / 2  per touched weight, the same form with c * A per
accumulator; every float outside the touched set bit-identical.  The two half ulps are the two roundings a float32 implementation cannot avoid (two
occurrences of a chained row: one each); c * M covers everything that depends on the ORDER of float32 sums: T, the logit and with it g.

WHERE C COMES FROM.  Not chosen: measured.  tests/test_ffm_ref_cpu.py runs the oracle itself through this judge on the probe sets of every shape
of MATRIX and of DIST_MATRIX (the multi-rank routes' sets, with and without duplicates) and takes the largest ratio (err - ulp(before) / 2 - ulp(after) / 2) / M it reaches on any weight, accumulator or LR entry
(the error beyond the unavoidable roundings: err / M alone has no maximum, ulp(w) / M grows without bound as the facing field's weights shrink).
C is 8 times that maximum -- room for a second correct float32 implementation (another order of the sums in T) and another summation tree for the logit.
Measured maximum: ORACLE_MAX_RATIO below, reached on the shape named next to it; test_oracle_stays_within_the_recorded_maximum fails if the oracle
ever exceeds it (then C is stale).  Probes with |p - y| < MIN_P_MINUS_Y are not judged (g = p - y carries the logit's absolute error, 1e-7 / |p - y|
relative); at most one probe in ten of a shape may be left out that way (asserted per shape).

PREDICTIONS have a constant of their own: |p - p_ref| <= min(C_P * M_p + 4 ulp(p), 5e-5), M_p = 1/4 * the sum of the |terms| of the logit as the
float64 pass forms them (|w v| per LR entry, |T[f][z] T[z][f]| per pair element, the halves of the diagonal and of the self pairs; logistic' <= 1/4;
expf, the sum and the division of 1 / (1 + expf(-t)) are good for 3 ulp together).  C_P is 8 times the largest (err - 4 ulp) / M_p the oracle reaches
on MATRIX's probe sets on EITHER of its forward passes (the learning pass and the predict-only one, which sums in another order): measured like C,
recorded as ORACLE_MAX_P_RATIO, and some four hundred times smaller than C -- the logit is a sum of float32 products and nothing divides by |p - y|.
The bound never exceeds the stream tests' 5e-5 (PRED_CAP).  A dropped pair element or a wrong self-pair term moves p by 1e-4 .. 1e-2 here and fails it
(planted in tests/test_ffm_ref_cpu.py).
"""
import numpy as np

from oracle import fwo

MIN_P_MINUS_Y = 0.05
MAX_SKIPPED_SHARE = 0.1
# the largest ratio the oracle reaches on MATRIX's probe sets (test_ffm_ref_cpu.py measures and asserts it); C = 8 x that
# (8.91e-6 on MATRIX's own sets, reached on 30x10; the multi-rank routes' probe set of 20x12 -- dist_probe_stream, with duplicates -- reaches 1.001e-5)
ORACLE_MAX_RATIO = 1.01e-5
ORACLE_MAX_RATIO_SHAPE = "20x12"
ORACLE_MAX_RATIO_SET = "dist"  # "matrix": probe_stream(F, k); "dist": dist_probe_stream(F, k, dup=True)
C = 8 * ORACLE_MAX_RATIO
# the same for predictions: the largest (err - 4 ulp) / M_p of the oracle's two forward passes; C_P = 8 x that
ORACLE_MAX_P_RATIO = 3.19e-8
ORACLE_MAX_P_RATIO_SHAPE = "65x2"
C_P = 8 * ORACLE_MAX_P_RATIO
PRED_CAP = 5e-5  # the stream tests' bar on a prediction: the one-step bound is never above it


class StepConfig:
    """the optimizer and its constants, with the oracle's own LUTs"""

    def __init__(self, optimizer, F, k, lr=0.1, ffm_lr=0.1, power_t=0.5, ffm_power_t=0.5, init_acc=1.0, ffm_init_acc=None):
        self.optimizer, self.F, self.k = int(optimizer), F, k
        self.lr, self.ffm_lr, self.power_t, self.ffm_power_t = (float(np.float32(x)) for x in (lr, ffm_lr, power_t, ffm_power_t))
        ffm_init_acc = init_acc if ffm_init_acc is None else ffm_init_acc
        om = fwo.Model(fwo.make_config(optimizer=self.optimizer, learning_rate=lr, power_t=power_t, init_acc_gradient=init_acc, bit_precision=4,
                                       ffm_k=0, ffm_bit_precision=4, ffm_learning_rate=ffm_lr, ffm_power_t=ffm_power_t,
                                       ffm_init_acc_gradient=ffm_init_acc), init=False)
        self.lut_lr, self.lut_ffm = om.lut("lr").astype(np.float64), om.lut("ffm").astype(np.float64)
        om.close()

    @classmethod
    def from_oracle_config(cls, ocfg):
        return cls(ocfg.optimizer, ocfg.ffm_num_fields, ocfg.ffm_k, ocfg.learning_rate, ocfg.ffm_learning_rate, ocfg.power_t, ocfg.ffm_power_t,
                   ocfg.init_acc_gradient, ocfg.ffm_init_acc_gradient)


def _lut_key(acc32):
    """optimizer.rs:147-156: the top 11 bits of the float below the sign"""
    return (np.asarray(acc32, dtype=np.float32).view(np.uint32) >> np.uint32(20)) & np.uint32(2047)


def _steps(optimizer, grad, acc, rate, power_t, lut, acc32_final):
    """one occurrence's steps on the running accumulators `acc` (float64, updated in place); acc32_final: the judged float32 new accumulators
    where this occurrence is the float's last (NaN elsewhere)"""
    if optimizer == fwo.OPT_SGD:
        return grad * rate
    acc += grad * grad
    if optimizer == fwo.OPT_ADAGRAD_FLEX:
        with np.errstate(all="ignore"):
            u = grad * rate * np.power(acc, -power_t)
        return np.where(np.isfinite(u), u, 0.0)
    a32 = np.where(np.isnan(acc32_final), acc.astype(np.float32), acc32_final).astype(np.float32)
    return grad * lut[_lut_key(a32)]


class StepRef:
    """what step() returns: p, g, logit, M_p; ffm_idx (sorted table floats the example touches), ffm_dw, ffm_dacc, ffm_M, ffm_A; lr_idx (sorted
    LR hashes), lr_dw, lr_dacc, lr_M, lr_A; updated (False: importance 0)"""


def forward(cfg, ffm_w, lr_tab, lr_ent, ffm_ent):
    """(logit, M_p, T, Tabs, rows): the float64 forward pass.  rows: (n, F, k) pre-update weights of the FFM entries"""
    F, k, R = cfg.F, cfg.k, cfg.F * cfg.k
    lr_w = lr_tab[2 * lr_ent["hash"].astype(np.int64)].astype(np.float64)
    lr_v = lr_ent["value"].astype(np.float64)
    logit = float(np.sum(lr_w * lr_v))
    mag = float(np.sum(np.abs(lr_w * lr_v)))
    n = len(ffm_ent)
    T = np.zeros((F, F, k))
    Tabs = np.zeros((F, F, k))
    rows = np.zeros((n, F, k))
    if k and n:
        h = ffm_ent["hash"].astype(np.int64)
        fld = (ffm_ent["contra_field_index"] // k).astype(np.int64)
        v = ffm_ent["value"].astype(np.float64)
        rows = ffm_w[h[:, None] + np.arange(R)[None, :]].astype(np.float64).reshape(n, F, k)
        np.add.at(T, fld, rows * v[:, None, None])
        np.add.at(Tabs, fld, np.abs(rows * v[:, None, None]))
        Tt = T.transpose(1, 0, 2)  # Tt[f][z] = T[z][f]
        pair = np.sum(T * Tt, axis=2)  # pair[f][z] = T[f][z] . T[z][f]
        low = np.tril(np.ones((F, F), dtype=bool), -1)
        selfp = np.zeros(F)
        np.add.at(selfp, fld, np.sum((rows[np.arange(n), fld] * v[:, None]) ** 2, axis=1))
        logit += float(np.sum(pair[low]) + 0.5 * (np.sum(np.diag(pair)) - np.sum(selfp)))
        mag += float(np.sum(np.sum(np.abs(T * Tt), axis=2)[low]) + 0.5 * (np.sum(np.diag(pair)) + np.sum(selfp)))  # (the diagonal's terms are squares)
    return logit, 0.25 * mag, T, Tabs, rows


def logistic(t):
    return 1.0 / (1.0 + np.exp(-t))


def predict(cfg, ffm_w, lr_tab, lr_ent, ffm_ent):
    """(p, M_p) of a read-only pass"""
    logit, M_p, _, _, _ = forward(cfg, ffm_w, lr_tab, lr_ent, ffm_ent)
    if np.isnan(logit):
        return 0.5, M_p
    return float(logistic(min(max(logit, -50.0), 50.0))), M_p


def step(cfg, ffm_w, ffm_acc, lr_tab, lr_ent, ffm_ent, label, importance, acc_after=None, lr_after=None):
    """One example's learning step on the float32 tables `ffm_w`, `ffm_acc`, `lr_tab` (interleaved {w, acc}), which are NOT changed.
    acc_after / lr_after: the judged implementation's tables after the step (AdagradLUT keys); None: the float64 sums rounded to float32."""
    F, k, R = cfg.F, cfg.k, cfg.F * cfg.k
    out = StepRef()
    logit, out.M_p, T, Tabs, rows = forward(cfg, ffm_w, lr_tab, lr_ent, ffm_ent)
    out.logit = logit
    if np.isnan(logit):
        out.p, g = 0.5, 0.0
    elif logit < -50.0 or logit > 50.0:
        out.p, g = float(logistic(np.sign(logit) * 50.0)), 0.0
    else:
        out.p = float(logistic(logit))
        g = -(float(label) - out.p) * float(importance)
    out.g = g
    out.updated = float(importance) != 0.0  # regressor.rs:356-379: an example of importance 0 is only predicted

    # ---- FFM rows, occurrence by occurrence in buffer order
    n = len(ffm_ent) if k else 0
    h = ffm_ent["hash"].astype(np.int64)[:n]
    flat = (h[:, None] + np.arange(R)[None, :]).reshape(-1) if n else np.zeros(0, dtype=np.int64)
    out.ffm_idx, inv = np.unique(flat, return_inverse=True)
    inv = inv.reshape(n, R) if n else inv
    m = len(out.ffm_idx)
    out.ffm_dw, out.ffm_dacc, out.ffm_M, out.ffm_A = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
    if n and out.updated:
        fld = (ffm_ent["contra_field_index"] // k).astype(np.int64)
        v = ffm_ent["value"].astype(np.float64)
        last = np.zeros(m, dtype=np.int64)
        for i in range(n):
            last[inv[i]] = i
        acc = ffm_acc[out.ffm_idx].astype(np.float64)
        acc0 = acc.copy()
        for i in range(n):
            f = fld[i]
            facing = T[:, f, :].copy()  # facing[z] = T[z][f]
            facing[f] -= rows[i, f] * v[i]
            grad = (g * v[i] * facing).reshape(-1)
            M = (cfg.ffm_lr * abs(g) * abs(v[i]) * Tabs[:, f, :]).reshape(-1)
            a = acc[inv[i]]
            final = np.full(R, np.nan, dtype=np.float32)
            if acc_after is not None:
                sel = last[inv[i]] == i
                final[sel] = acc_after[out.ffm_idx[inv[i]][sel]]
            u = _steps(cfg.optimizer, grad, a, cfg.ffm_lr, cfg.ffm_power_t, cfg.lut_ffm, final)
            acc[inv[i]] = a
            np.add.at(out.ffm_dw, inv[i], -u)
            np.add.at(out.ffm_M, inv[i], M)
            np.add.at(out.ffm_A, inv[i], 2.0 * np.abs(grad) * M / cfg.ffm_lr)
        out.ffm_dacc = acc - acc0

    # ---- LR entries, in buffer order (a hash that occurs twice is stepped twice on its running accumulator)
    lh = lr_ent["hash"].astype(np.int64)
    out.lr_idx, linv = np.unique(lh, return_inverse=True)
    m = len(out.lr_idx)
    out.lr_dw, out.lr_dacc, out.lr_M, out.lr_A = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
    if out.updated:
        lv = lr_ent["value"].astype(np.float64)
        acc = lr_tab[2 * out.lr_idx + 1].astype(np.float64)
        acc0 = acc.copy()
        llast = np.zeros(m, dtype=np.int64)
        llast[linv] = np.arange(len(lh))
        for i in range(len(lh)):
            j = linv[i]
            grad = np.array([g * lv[i]])
            a = acc[j:j + 1]
            final = np.array([lr_after[2 * lh[i] + 1] if lr_after is not None and llast[j] == i else np.nan], dtype=np.float32)
            u = _steps(cfg.optimizer, grad, a, cfg.lr, cfg.power_t, cfg.lut_lr, final)
            M = cfg.lr * abs(g) * abs(lv[i])
            out.lr_dw[j] -= u[0]
            out.lr_M[j] += M
            out.lr_A[j] += 2.0 * abs(grad[0]) * M / cfg.lr
        out.lr_dacc = acc - acc0
    return out


def _ulp(x32):
    return np.spacing(np.abs(np.asarray(x32, dtype=np.float32))).astype(np.float64)


def judge_floats(before, after, delta, M):
    """(err, slack, M): err = |after - (before + delta)| in float64, slack = ulp(before) / 2 + ulp(after) / 2; the judge is err <= c * M + slack"""
    b, a = np.asarray(before, dtype=np.float32), np.asarray(after, dtype=np.float32)
    err = np.abs(a.astype(np.float64) - (b.astype(np.float64) + delta))
    return err, 0.5 * _ulp(b) + 0.5 * _ulp(a), np.asarray(M, dtype=np.float64)


def ratio(err, slack, M):
    """the c a float would need: (err - slack) / M, 0 where err <= slack, inf where the error exceeds the roundings on a float whose M is 0"""
    ex = np.maximum(err - slack, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ex == 0.0, 0.0, np.where(M > 0.0, ex / M, np.inf))


class Verdict:
    """judge_example's result: `worst` = the largest c any float of the example needs, `where` = (table, index, err, bound at C) of that float,
    `skipped` (|p - y| < MIN_P_MINUS_Y: only the prediction was judged), the ratios per table (w, acc, lr_w, lr_acc), and the prediction's own
    verdict: p_err <= p_bound is the judge, p_ratio the c_p it needs (judge_prediction)"""


def judge_example(cfg, before, after, lr_ent, ffm_ent, label, importance, p_got):
    """before / after: (ffm_w, ffm_acc, lr_tab) float32 tables around ONE example's step of the judged implementation; p_got its prediction."""
    w0, a0, l0 = before
    w1, a1, l1 = after
    ref = step(cfg, w0, a0, l0, lr_ent, ffm_ent, label, importance, acc_after=a1, lr_after=l1)
    v = Verdict()
    v.ref = ref
    p32 = np.float32(p_got)
    v.p_err, v.p_bound, v.p_ratio = judge_prediction(p32, ref.p, ref.M_p)
    v.ratios = {}
    v.skipped = ref.updated and ref.g != 0.0 and abs(ref.p - float(label)) < MIN_P_MINUS_Y
    if not v.skipped:
        i, j = ref.ffm_idx, ref.lr_idx
        v.ratios["w"] = ratio(*judge_floats(w0[i], w1[i], ref.ffm_dw, ref.ffm_M))
        v.ratios["acc"] = ratio(*judge_floats(a0[i], a1[i], ref.ffm_dacc, ref.ffm_A))
        v.ratios["lr_w"] = ratio(*judge_floats(l0[2 * j], l1[2 * j], ref.lr_dw, ref.lr_M))
        v.ratios["lr_acc"] = ratio(*judge_floats(l0[2 * j + 1], l1[2 * j + 1], ref.lr_dacc, ref.lr_A))
    v.worst, v.where = 0.0, None
    for name, r in v.ratios.items():
        if len(r) and float(r.max()) > v.worst:
            v.worst = float(r.max())
            at = int(r.argmax())
            v.where = (name, int({"w": ref.ffm_idx, "acc": ref.ffm_idx, "lr_w": ref.lr_idx, "lr_acc": ref.lr_idx}[name][at]))
    return v


def judge_prediction(p_got, p_ref, M_p):
    """(err, bound, the c_p the prediction needs): bound = min(C_P * M_p + 4 ulp(p), PRED_CAP)"""
    p32 = np.float32(p_got)
    err, slack = abs(float(p32) - float(p_ref)), 4.0 * float(_ulp(p32))
    need = 0.0 if err <= slack else ((err - slack) / M_p if M_p > 0.0 else np.inf)
    return err, min(C_P * M_p + slack, PRED_CAP), need


def untouched_identical(before, after, touched):
    """every float of the table outside `touched` (indices) is bit-identical"""
    b, a = np.asarray(before, dtype=np.float32).view(np.uint32), np.asarray(after, dtype=np.float32).view(np.uint32)
    diff = np.flatnonzero(b != a)
    return bool(np.all(np.isin(diff, touched)))


def old_bar(got, ref, weight_tol=2e-5):
    """the bar of the stream tests (helpers.stream_parity): |got - ref| <= 2e-5 + 1e-5 |ref|"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(got - ref) <= weight_tol + 1e-5 * np.abs(ref)))


# ------------------------------------------------------------------ probe sets: the shapes, their streams and their warm state
LUT, FLEX, SGD = fwo.OPT_ADAGRAD_LUT, fwo.OPT_ADAGRAD_FLEX, fwo.OPT_SGD
# (F, k): every shape of tests/test_gpu_ffm_step.py's matrix (the launch options a shape is run under do not change its probe set)
MATRIX = [(30, 10), (65, 2), (30, 3), (65, 1),                                   # scalar kernel
          (6, 4), (30, 8),                                                       # ... chosen because rows are not 16-byte aligned
          (20, 12), (21, 12), (12, 20), (10, 24),                                # register-resident kernel, k not a power of two
          (8, 32), (2, 128), (16, 32), (4, 128), (5, 64),                        # ... large k
          (30, 12), (21, 24), (40, 16), (25, 32), (20, 64), (10, 4),             # generic 16-byte kernel
          (30, 16), (40, 8)]                                                     # shapes the stream tests run
N_PROBES = 20


def probe_stream(F, k, seed=None):
    """the shape's probe set: N_PROBES examples that share nothing (helpers.disjoint_stream), with chained duplicates, weighted features, fields of
    0..2 features (F >= 8: an EMPTY field among them) and -- wherever F < 8 -- fewer features than a workgroup has waves"""
    from helpers import disjoint_stream

    return disjoint_stream(F, k, N_PROBES, per_field=(0, 2) if F >= 8 else (1, 2), p_weighted=0.3, p_dup=0.15, seed=1000 + 7 * F + k if seed is None else seed)


# (F, k) of tests/test_gpu_dist_step.py: the smallest shapes at which each branch of the split, peer-sharded and owner-side routes is taken
DIST_MATRIX = [(6, 4),     # R = 24: the base case; fewer features than waves
               (30, 8),    # R = 240: config C; one full 16-byte chunk
               (30, 3),    # R = 90: VEC = 1 phases and push; the scalar apply and consume paths, two trips of 64
               (30, 10),   # R = 300: the same with five chunks
               (20, 12),   # R = 240: e0 / k a real division in the push and the phases
               (5, 64),    # R = 320: a nearly empty second chunk; the owner apply's second trip; the consumer's chunk c = 1
               (16, 32),   # R = 512: two full chunks; the consumer's early slot hand-back at its limit
               (30, 16),   # R = 480: the largest shape whose phases still stage T in LDS
               (40, 16)]   # R = 640: three chunks; the consumer's e0 >= 512 tail and late hand-back; the owner apply's third trip; T in the split record
# per shape: what is added to the probe set's seed until the float64 reference leaves out at most MAX_SKIPPED_SHARE of it (test_ffm_ref_cpu.py asserts the share)
DIST_SEED_BUMP = {}


def dist_probe_stream(F, k, dup=True):
    """the shape's probe set for the multi-rank routes: probe_stream's draw (seeds of its own) with the rows dealt over the four quarters of the
    table (helpers.disjoint_stream scatter = 4: every example of four or more features has rows at every owner of a 2- or 4-rank job, no row
    crosses an ownership boundary).  dup = False: no chained duplicates -- for the concurrent owner-side routes, where two occurrences of one row
    are pushed and applied by different waves and race inside the owner by design."""
    from helpers import disjoint_stream

    seed = (2000 if dup else 3000) + 7 * F + k + DIST_SEED_BUMP.get((F, k, dup), 0)
    return disjoint_stream(F, k, N_PROBES, per_field=(0, 2) if F >= 8 else (1, 2), p_weighted=0.3, p_dup=0.15 if dup else 0.0, scatter=4, seed=seed)


def warm_state(st, seed=5):
    """(ffm_w, ffm_acc, lr_tab) float32 over the stream's span: weights of a size that makes the logits O(1) (uniform in +-s, s^2 / 3 * sqrt(pairs * k)
    = 0.45), accumulators drawn from [1, 4] (LUT keys and powf arguments vary), LR weights in +-0.6 / sqrt(F)"""
    rng = np.random.default_rng(seed + 31 * st.F + st.k)
    pairs = max(1, st.F * (st.F - 1) // 2) * st.k
    s = np.sqrt(1.35 / np.sqrt(pairs)) * (0.6 if st.F < 8 else 1.0)  # (F < 8: no field is empty, see probe_stream -- half again as many features)
    n = st.span + st.R
    w = rng.uniform(-s, s, n).astype(np.float32)
    acc = rng.uniform(1.0, 4.0, n).astype(np.float32)
    lr = np.empty(2 * st.span, dtype=np.float32)
    lr[0::2] = rng.uniform(-0.6, 0.6, st.span) / np.sqrt(st.n_ns)
    lr[1::2] = rng.uniform(1.0, 4.0, st.span)
    return w, acc, lr


def opt_kwargs(opt):
    """the models' constants per optimizer, as the stream tests choose them"""
    return dict(lr=0.05, ffm_lr=0.05) if opt == SGD else {}
