"""One learning step of ONE example through the deep head in float64, and the judge that compares a float32 implementation with it.

A numpy restatement of `chain_nn` of oracle/fw_oracle.c for one example, from float32 before-tables (LR, FFM_W, FFM_ACC, NN_W, NN_ACC), composed of the pieces
the suite already has: head_ref.head_inputs64 (x and the sums of absolute products behind every slot), the n = 1 case of head_ref.head_train64 (pre, mask, z, p,
g, the per-layer output gradients, dx) and ffm_ref._steps / judge_floats / ratio (the optimizer steps and the per-float judge).  It is to the per-example head of
csrc/kernels.hip (nn_forward / nn_backward / nn_layer_backward / nn_layer_backward_vec, a phase of fw_example_kernel<..., NN = true> and of
fw_example_kernel_r<..., NN = true>) what ffm_ref.py is to the headless kernels.

    forward     x = [per-combo LR sums | triangle of the FFM pair outputs]; hidden layers pre = W h + b, ReLU mask = [pre >= 0] or identity; the final neuron over
                [h_last | x] (topology one) or h_last (topology two); p = logistic(z); g = (p - y) * importance.
    dense       layer by layer from the final neuron down.  A unit whose output gradient og[j] is EXACTLY 0 (a dead ReLU unit, or every unit above it dead) leaves
                its weight row, its bias and their accumulators untouched.  Otherwise weight (j, i) takes gradient og[j] * in[i], the bias og[j]; the step is
                ffm_ref._steps (AdagradLUT: the key from the judged implementation's own float32 new accumulator).  A weight whose input is exactly 0 has a
                zero gradient and must keep its value whatever the table holds at its key (0 * lut[0]).
    input grad  from the PRE-update weights: d in = og . W_old; in topology one the final neuron's direct part g * w_f[wl:] is added (BlockCopy sums both branches).
    sparse      LR entry t takes dx[combo_t] * v_t.  FFM occurrence i of field f, float (z, kk), takes dx[C + tri(f, z)] * v_i * (T[z][f] - [z == f] w_i v_i), tri
                the mirror of fwo_triangle_backward (the factor 2 of the way forward does NOT come back); w always the pre-update weight; chained duplicates in
                buffer order on a running accumulator, as in ffm_ref.step.

MAGNITUDES.  Every quantity q of the pass carries S(q), the propagated sum of absolute products behind it: S(x_i) is head_inputs64's sum_abs, a sum adds the S of
its terms, a product multiplies them (S(w) = |w| for a table float), a mask passes or zeroes; S(g) = |g| (as in ffm_ref: the logit's error in g is what the probes
with a small |p - y| are left out for).  A stepped float's M is its table's rate times S(gradient): nn_lr * S(og_j) * S(in_i) for a dense weight, nn_lr * S(og_j)
for a bias, lr * S(dx_combo) * |v| for an LR entry, ffm_lr * S(dx_t) * |v_i| * sum_i' |v_i'| |w_i'| for an FFM float (the sum behind T[z][f], as in ffm_ref), summed
over a float's occurrences; its accumulator's A = sum 2 |grad| M / rate.

THE JUDGE is ffm_ref.judge_floats, per stepped float of all five tables:  |after - (before + d_ref)| <= c * M + ulp(before) / 2 + ulp(after) / 2  (c * A for an
accumulator); every other float bit-identical (ffm_ref.untouched_identical).  The prediction: |p - p64| <= C_P * 0.25 * t_z + 4 ulp(p), t_z the forward bound on the
logit that head_train64 propagates (every stage adds head_ref.dot_bound of its own sums to what its inputs carry), started from dot_bound(S(x)) for the slots of
x that are sums at all.

WHERE THE CONSTANTS COME FROM.  Measured: tests/test_deep_step_ref_cpu.py runs the ORACLE through this judge on every case of CASES and takes the largest
(err - slack) / M it reaches -- one maximum for the dense tables, one for the sparse tables behind the head, one for the prediction.  Each constant is 8 times its
maximum (ffm_ref.C's margin, for the same reason: room for a second correct float32 order of the sums).  The maxima and the cases that reached them stand next to
the constants below; the CPU test fails if the oracle ever exceeds one.

PROBES LEFT OUT.  By the reference alone: a probe with a ReLU unit whose |pre64| <= RELU_MARGIN * dot_bound(sum |w| |in| + |b|) is rejected (float32 and float64
may disagree about that unit's mask: head_ref.draw_train_case's rule, on the unit's own sum as there); a probe with |p - y| < MIN_P_MINUS_Y has only its prediction judged.  A case may lose at most one probe
in ten either way; the seeds of CASES are picked so that every case stays inside that (asserted in the CPU test)."""
import numpy as np

import ffm_ref
import fwumious_wabbit_amd as fw
from ffm_ref import FLEX, LUT, SGD, judge_floats, ratio, untouched_identical
from head_ref import (RELU_MARGIN, SHAPES, Entries, dense_head_weights, dot_bound, head_inputs64, head_layout, head_train64)
from helpers import disjoint_stream, make_pair
from oracle import fwo

MIN_P_MINUS_Y = ffm_ref.MIN_P_MINUS_Y
Z_MAX = 2.5  # the largest |logit| of a case's probes: |p - y| >= 0.075, so no probe of CASES is left out for a small |p - y|
MAX_REJECTED = 0.1
MAX_SKIPPED_SHARE = 0.1
# the largest ratios the oracle reaches on CASES (test_deep_step_ref_cpu.py measures and asserts them); each constant is 8 x its maximum
ORACLE_MAX_DENSE_RATIO = 1.40e-6
ORACLE_MAX_DENSE_RATIO_CASE = "g_sgd"
C_DENSE = 8 * ORACLE_MAX_DENSE_RATIO
ORACLE_MAX_SPARSE_RATIO = 7.54e-7
ORACLE_MAX_SPARSE_RATIO_CASE = "a_init0"
C_SPARSE = 8 * ORACLE_MAX_SPARSE_RATIO
ORACLE_MAX_P_RATIO = 1.63e-4
ORACLE_MAX_P_RATIO_CASE = "a_init0"
C_P = 8 * ORACLE_MAX_P_RATIO

TABLE_NAMES = ("LR", "FFM_W", "FFM_ACC", "NN_W", "NN_ACC")  # the order of every `before` / `after` tuple of this module


# ------------------------------------------------------------------ the cases: shape, head, optimizer, probe count and seed
def _case(F, k, layers, topo="one", inter=(), opt=LUT, nn_init_acc=1.0, n=6, seed=0):
    return dict(F=F, k=k, layers=list(layers), topo=topo, inter=list(inter), opt=opt, nn_init_acc=nn_init_acc, n=n, seed=seed)


_A, _G, _D = SHAPES["a"], SHAPES["c"], SHAPES["d"]
CASES = {
    "a": _case(_A["F"], _A["k"], _A["layers"], _A["topo"], _A["inter"], seed=100),
    "a_init0": _case(_A["F"], _A["k"], _A["layers"], _A["topo"], _A["inter"], nn_init_acc=0.0, seed=200),
    "b": _case(7, 4, [(64, "relu"), (8, "relu")], seed=301),
    "b64": _case(7, 4, [(64, "relu"), (64, "relu")], seed=400),
    "c": _case(7, 4, [(65, "relu"), (65, "relu")], seed=500),
    "d": _case(7, 4, [(516, "relu")], seed=600),
    "e": _case(_D["F"], _D["k"], _D["layers"], _D["topo"], seed=700),
    "f_5x16": _case(5, 16, [(25, "relu")], seed=800),
    "f_3x5": _case(3, 5, [(9, "none"), (7, "relu")], "two", seed=900),
    "g": _case(_G["F"], _G["k"], _G["layers"], _G["topo"], n=4, seed=1004),
    "a_sgd": _case(_A["F"], _A["k"], _A["layers"], _A["topo"], _A["inter"], opt=SGD, seed=1100),
    "a_flex": _case(_A["F"], _A["k"], _A["layers"], _A["topo"], _A["inter"], opt=FLEX, seed=1200),
    "g_sgd": _case(_G["F"], _G["k"], _G["layers"], _G["topo"], opt=SGD, n=4, seed=1305),
    "g_flex": _case(_G["F"], _G["k"], _G["layers"], _G["topo"], opt=FLEX, n=4, seed=1403),
}


class DeepConfig:
    """the model's constants: `sparse` (ffm_ref.StepConfig of the LR and FFM blocks), C combos, the head (layers [(width, activation)], topo), the dense rate,
    power and the oracle's own LUT for the dense tables"""

    def __init__(self, ocfg, layers, topo, nn_lr, nn_power_t, nn_init_acc):
        self.sparse = ffm_ref.StepConfig.from_oracle_config(ocfg)
        self.optimizer, self.F, self.k, self.C = int(ocfg.optimizer), int(ocfg.ffm_num_fields), int(ocfg.ffm_k), int(ocfg.num_combos)
        self.layers, self.topo = [(w, a) for w, a in layers], topo
        self.X = self.C + self.F * (self.F + 1) // 2
        self.lay, self.total = head_layout(self.X, self.layers, topo)
        self.nn_lr, self.nn_power_t = float(np.float32(nn_lr)), float(np.float32(nn_power_t))
        dense = ffm_ref.StepConfig(self.optimizer, 0, 0, lr=nn_lr, power_t=nn_power_t, init_acc=nn_init_acc)
        self.lut_nn = dense.lut_lr

    def locate(self, idx):
        """(layer, unit, input) of float `idx` of the dense tables; input -1: the unit's bias"""
        for l, (o, out, w_in) in enumerate(self.lay):
            if idx < o + out * w_in:
                return l, (idx - o) // w_in, (idx - o) % w_in
            if idx < o + out * w_in + out:
                return l, idx - o - out * w_in, -1
        raise IndexError(idx)


def tri(i, j):
    """the slot of the field pair (i, j) in the triangle, either order: fwo_triangle_backward's mirror"""
    i, j = np.maximum(i, j), np.minimum(i, j)
    return i * (i + 1) // 2 + j


class StepRef:
    """what step() returns.  Forward: x, sa_x, exact0, tr (head_train64's dict), p, g, t_z, rejected, skipped, og / S_og (per layer, the final neuron last), dx, S_dx.
    Dense: nn_idx (sorted floats of the live units' rows and biases), nn_dw, nn_dacc, nn_M, nn_A.  Sparse: ffm_idx, ffm_dw, ffm_dacc, ffm_M, ffm_A; lr_idx, lr_dw,
    lr_dacc, lr_M, lr_A (as ffm_ref.StepRef)."""


def step(cfg, before, lr_ent, ffm_ent, label, importance, after=None, plant=None):
    """One example's step from the float32 tables `before` = (LR, FFM_W, FFM_ACC, NN_W, NN_ACC), which are not changed.  `after`: the judged implementation's tables
    after the step (the AdagradLUT keys); None: the float64 sums rounded to float32.  `plant` (tests/test_deep_step_ref_cpu.py): the step a subtly wrong kernel
    would take -- "post_update_dx": the direct part of dx from the final neuron's POST-update weights; "tri_neighbour": the row gradient of field f's slot z from
    dx[C + tri(z, f + 1)]; "lr_takes_g": the LR entries stepped with g instead of dx[combo]."""
    lr_tab, ffm_w, ffm_acc, nn_w, nn_acc = before
    F, k, C, X, L, opt = cfg.F, cfg.k, cfg.C, cfg.X, len(cfg.layers), cfg.optimizer
    out = StepRef()
    en = Entries([np.asarray(lr_ent)], [np.asarray(ffm_ent)])
    x, sa_x, exact0 = head_inputs64(lr_tab, ffm_w, C, F, k, en)
    out.x, out.sa_x, out.exact0 = x[0], sa_x[0], exact0[0]
    tr = out.tr = head_train64(x, [[float(label), float(importance)]], nn_w, cfg.layers, cfg.topo)
    W64 = np.asarray(nn_w, dtype=np.float64)
    Ws = [W64[o:o + o_n * w_in].reshape(o_n, w_in) for o, o_n, w_in in cfg.lay]
    bs = [W64[o + o_n * w_in:o + o_n * w_in + o_n] for o, o_n, w_in in cfg.lay]
    masks = [tr["mask"][l][0] for l in range(L)]
    hs = [tr["h"][l][0] for l in range(L)]
    wl = cfg.lay[-2][1]

    # ---- forward: S of every unit, the ReLU margin, the bound on the logit
    S_in, t_in = out.sa_x, np.where(out.exact0, 0.0, dot_bound(out.sa_x))
    S_h, near = [], False
    hin = out.x
    for l in range(L):
        S_pre = S_in @ np.abs(Ws[l]).T + np.abs(bs[l])
        own = dot_bound(np.abs(hin) @ np.abs(Ws[l]).T + np.abs(bs[l]))
        if cfg.layers[l][1] == "relu":
            near = near or bool(np.any(np.abs(tr["pre"][l][0]) <= RELU_MARGIN * own))
        t_in = (own + t_in @ np.abs(Ws[l]).T) * masks[l]
        S_h.append(S_pre * masks[l])
        S_in, hin = S_h[-1], hs[l]
    one = cfg.topo == "one"
    fx = np.concatenate([hin, out.x]) if one else hin
    S_fx = np.concatenate([S_in, out.sa_x]) if one else S_in
    t_fx = np.concatenate([t_in, np.where(out.exact0, 0.0, dot_bound(out.sa_x))]) if one else t_in
    wf, bf = Ws[L][0], bs[L][0]
    out.t_z = float(dot_bound(np.abs(fx) @ np.abs(wf) + abs(bf)) + t_fx @ np.abs(wf))
    out.z, out.p, g = float(tr["z"][0]), float(tr["p"][0]), float(tr["g"][0])
    out.g, out.rejected = g, near
    out.updated = float(importance) != 0.0
    out.skipped = out.updated and g != 0.0 and abs(out.p - float(label)) < MIN_P_MINUS_Y

    # ---- backward: output gradients per layer and their S, the input gradient from the PRE-update weights
    og, S_og = [None] * (L + 1), [None] * (L + 1)
    og[L], S_og[L] = np.array([g]), np.array([abs(g)])
    S_d = abs(g) * np.abs(wf[:wl]) * masks[L - 1]
    S_direct = abs(g) * np.abs(wf[wl:]) if one else np.zeros(X)
    for l in range(L - 1, -1, -1):
        og[l], S_og[l] = tr["dz"][l][0], S_d
        S_din = S_d @ np.abs(Ws[l])
        if l > 0:
            S_d = S_din * masks[l - 1]
    out.og, out.S_og = og, S_og
    out.dx, out.S_dx = tr["dx"][0].copy(), S_direct + S_din

    # ---- dense steps, the final neuron first (the order does not matter: no float is stepped twice)
    ins = [out.x] + hs[:-1] + [fx]
    S_ins = [out.sa_x] + S_h[:-1] + [S_fx]
    idxs, dws, daccs, Ms, As = [], [], [], [], []
    for l, (o, o_n, w_in) in enumerate(cfg.lay):
        live = og[l] != 0.0
        if not out.updated or not np.any(live):
            continue
        sel = np.concatenate([np.repeat(live, w_in), live])
        grad = np.concatenate([(og[l][:, None] * ins[l][None, :]).reshape(-1), og[l]])[sel]
        S = np.concatenate([(S_og[l][:, None] * S_ins[l][None, :]).reshape(-1), S_og[l]])[sel]
        idx = o + np.flatnonzero(sel)
        acc = np.asarray(nn_acc)[idx].astype(np.float64)
        acc0 = acc.copy()
        final = np.asarray(after[4])[idx].astype(np.float32) if after is not None else np.full(len(idx), np.nan, dtype=np.float32)
        u = ffm_ref._steps(opt, grad, acc, cfg.nn_lr, cfg.nn_power_t, cfg.lut_nn, final)
        M = cfg.nn_lr * S
        idxs.append(idx), dws.append(-u), daccs.append(acc - acc0), Ms.append(M), As.append(2.0 * np.abs(grad) * M / cfg.nn_lr)
    cat = lambda parts, dt=np.float64: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)
    out.nn_idx = cat(idxs, np.int64).astype(np.int64)
    out.nn_dw, out.nn_dacc, out.nn_M, out.nn_A = cat(dws), cat(daccs), cat(Ms), cat(As)
    order = np.argsort(out.nn_idx)
    out.nn_idx, out.nn_dw, out.nn_dacc, out.nn_M, out.nn_A = (a[order] for a in (out.nn_idx, out.nn_dw, out.nn_dacc, out.nn_M, out.nn_A))

    dx, S_dx = out.dx, out.S_dx
    if plant == "post_update_dx":
        assert one and g != 0.0
        o, _, fin = cfg.lay[L]
        wf_new = wf.copy()
        pos = np.searchsorted(out.nn_idx, o + np.arange(fin))
        wf_new += out.nn_dw[pos]
        dx = dx + g * (wf_new - wf)[wl:]

    # ---- FFM rows, occurrence by occurrence in buffer order (ffm_ref.step with the slot's own general gradient)
    sp = cfg.sparse
    R = F * k
    n = len(ffm_ent) if k else 0
    h = ffm_ent["hash"].astype(np.int64)[:n]
    flat = (h[:, None] + np.arange(R)[None, :]).reshape(-1) if n else np.zeros(0, dtype=np.int64)
    out.ffm_idx, inv = np.unique(flat, return_inverse=True)
    inv = inv.reshape(n, R) if n else inv
    m = len(out.ffm_idx)
    out.ffm_dw, out.ffm_dacc, out.ffm_M, out.ffm_A = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
    if n and out.updated:
        _, _, T, Tabs, rows = ffm_ref.forward(sp, ffm_w, lr_tab, lr_ent, ffm_ent)
        fld = (ffm_ent["contra_field_index"] // k).astype(np.int64)
        v = ffm_ent["value"].astype(np.float64)
        last = np.zeros(m, dtype=np.int64)
        for i in range(n):
            last[inv[i]] = i
        acc = np.asarray(ffm_acc)[out.ffm_idx].astype(np.float64)
        acc0 = acc.copy()
        zs = np.arange(F)
        for i in range(n):
            f = int(fld[i])
            slot = C + tri(zs, (f + 1) % F if plant == "tri_neighbour" else f)
            facing = T[:, f, :].copy()  # facing[z] = T[z][f]
            facing[f] -= rows[i, f] * v[i]
            grad = (dx[slot][:, None] * v[i] * facing).reshape(-1)
            M = (sp.ffm_lr * S_dx[slot][:, None] * abs(v[i]) * Tabs[:, f, :]).reshape(-1)
            a = acc[inv[i]]
            final = np.full(R, np.nan, dtype=np.float32)
            if after is not None:
                s_ = last[inv[i]] == i
                final[s_] = np.asarray(after[2])[out.ffm_idx[inv[i]][s_]]
            u = ffm_ref._steps(opt, grad, a, sp.ffm_lr, sp.ffm_power_t, sp.lut_ffm, final)
            acc[inv[i]] = a
            np.add.at(out.ffm_dw, inv[i], -u)
            np.add.at(out.ffm_M, inv[i], M)
            np.add.at(out.ffm_A, inv[i], 2.0 * np.abs(grad) * M / sp.ffm_lr)
        out.ffm_dacc = acc - acc0

    # ---- LR entries in buffer order
    lh = lr_ent["hash"].astype(np.int64)
    combo = lr_ent["combo_index"].astype(np.int64)
    out.lr_idx, linv = np.unique(lh, return_inverse=True)
    m = len(out.lr_idx)
    out.lr_dw, out.lr_dacc, out.lr_M, out.lr_A = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
    if out.updated:
        lv = lr_ent["value"].astype(np.float64)
        acc = np.asarray(lr_tab)[2 * out.lr_idx + 1].astype(np.float64)
        acc0 = acc.copy()
        llast = np.zeros(m, dtype=np.int64)
        llast[linv] = np.arange(len(lh))
        for i in range(len(lh)):
            j = linv[i]
            general, S_general = (g, abs(g)) if plant == "lr_takes_g" else (dx[combo[i]], S_dx[combo[i]])
            grad = np.array([general * lv[i]])
            a = acc[j:j + 1]
            final = np.array([after[0][2 * lh[i] + 1] if after is not None and llast[j] == i else np.nan], dtype=np.float32)
            u = ffm_ref._steps(opt, grad, a, sp.lr, sp.power_t, sp.lut_lr, final)
            M = sp.lr * S_general * abs(lv[i])
            out.lr_dw[j] -= u[0]
            out.lr_M[j] += M
            out.lr_A[j] += 2.0 * abs(grad[0]) * M / sp.lr
        out.lr_dacc = acc - acc0
    return out


class Verdict:
    """judge_example's result: ref (StepRef); rejected / skipped (the reference's own decisions); p_err, p_bound (at C_P), p_ratio (the c_p the prediction needs);
    dense / sparse: the largest c a float of those tables needs, where_dense / where_sparse: a description of that float; untouched: None, or the name of a table
    in which a float outside the stepped set changed"""


def judge_prediction(p_got, ref):
    p32 = np.float32(p_got)
    err, slack, M_p = abs(float(p32) - ref.p), 4.0 * float(ffm_ref._ulp(p32)), 0.25 * ref.t_z
    return err, C_P * M_p + slack, (0.0 if err <= slack else (err - slack) / M_p)


def judge_example(cfg, before, after, lr_ent, ffm_ent, label, importance, p_got):
    """before / after: the five float32 tables around ONE example's step of the judged implementation; p_got its prediction"""
    ref = step(cfg, before, lr_ent, ffm_ent, label, importance, after=after)
    v = Verdict()
    v.ref, v.rejected, v.skipped = ref, ref.rejected, ref.skipped
    v.p_err, v.p_bound, v.p_ratio = judge_prediction(p_got, ref)
    v.dense, v.sparse, v.where_dense, v.where_sparse, v.untouched = 0.0, 0.0, None, None, None
    sgd = cfg.optimizer == SGD
    none = np.zeros(0, dtype=np.int64)
    touched = (np.concatenate([2 * ref.lr_idx] + ([] if sgd else [2 * ref.lr_idx + 1])), ref.ffm_idx, none if sgd else ref.ffm_idx, ref.nn_idx,
               none if sgd else ref.nn_idx)
    if v.rejected:  # (the masks may differ: nothing but the prediction can be judged)
        return v
    for name, b, a, t in zip(TABLE_NAMES, before, after, touched):
        if v.untouched is None and not untouched_identical(b, a, t):
            v.untouched = name
    if v.skipped:
        return v
    i, j, d = ref.ffm_idx, ref.lr_idx, ref.nn_idx
    lr0, w0, a0, n0, na0 = before
    lr1, w1, a1, n1, na1 = after
    parts = {"NN_W": (ratio(*judge_floats(n0[d], n1[d], ref.nn_dw, ref.nn_M)), d), "NN_ACC": (ratio(*judge_floats(na0[d], na1[d], ref.nn_dacc, ref.nn_A)), d),
             "FFM_W": (ratio(*judge_floats(w0[i], w1[i], ref.ffm_dw, ref.ffm_M)), i), "FFM_ACC": (ratio(*judge_floats(a0[i], a1[i], ref.ffm_dacc, ref.ffm_A)), i),
             "LR w": (ratio(*judge_floats(lr0[2 * j], lr1[2 * j], ref.lr_dw, ref.lr_M)), j),
             "LR acc": (ratio(*judge_floats(lr0[2 * j + 1], lr1[2 * j + 1], ref.lr_dacc, ref.lr_A)), j)}
    for name, (r, idx) in parts.items():
        if not len(r):
            continue
        at, worst = int(r.argmax()), float(r.max())
        if name.startswith("NN"):
            if worst > v.dense:
                l, unit, inp = cfg.locate(int(idx[at]))
                v.dense, v.where_dense = worst, f"{name} float {int(idx[at])}: layer {l}, unit {unit}, {'bias' if inp < 0 else 'input %d' % inp}"
        elif worst > v.sparse:
            v.sparse = worst
            if name.startswith("FFM"):
                rows_h = ffm_ent["hash"].astype(np.int64)
                row = int(rows_h[(rows_h <= idx[at]) & (idx[at] < rows_h + cfg.F * cfg.k)][0])
                v.where_sparse = f"{name} float {int(idx[at])}: row at {row}, float {int(idx[at]) - row} = field slot {(int(idx[at]) - row) // cfg.k}"
            else:
                v.where_sparse = f"{name} entry {int(idx[at])}"
    return v


def passes(v):
    """the judge at the module's constants"""
    return v.untouched is None and v.p_err <= v.p_bound and (v.rejected or v.skipped or (v.dense <= C_DENSE and v.sparse <= C_SPARSE))


# ------------------------------------------------------------------ a case's probes and the state the tests write
class Case:
    """build_case's result: st (the disjoint stream), mi / ocfg / ots / nn (the device's and the oracle's models), cfg (DeepConfig), fbs (the entry route's
    buffers), lr / ffm_w / ffm_acc / nn_w (float32 tables, written once per case) and nn_acc[e] (per probe)"""


_BUILT = {}


def opt_kwargs(opt):
    return dict(lr=0.05, ffm_lr=0.05) if opt == SGD else {}


def initial_acc(opt, init):
    return float(init) if opt == FLEX else 0.0  # (AdagradLUT folds the initial value into its table)


def build_case(name):
    """the case's probes, models and written state, built once and left unchanged.  Probes: helpers.disjoint_stream (weighted features, chained duplicates, fields of
    0 / 1 / 2 features); the models carry the constant feature and the case's interactions, which is fine here because every probe is launched alone from a state
    the test wrote.  Sparse warm state: ffm_ref.warm_state over the rows' span, the LR table written whole (the constant's and the interactions' entries lie
    anywhere in it).  Dense weights: head_ref.dense_head_weights on the probes' own x.  NN_ACC: log-uniform over [1, 64] (48 LUT buckets), a quarter of the
    floats left at the optimizer's initial value; where nn_init_acc_gradient is 0 an accumulator stays at 0 only where its gradient is exactly zero
    (an input that is exactly 0: there 0 * lut[0] must leave the weight alone) -- a first step of rate * g^(1 - 2 power_t) is not what M = rate * S(g) describes."""
    if name in _BUILT:
        return _BUILT[name]
    c = CASES[name]
    F, k, opt = c["F"], c["k"], c["opt"]
    cs = Case()
    cs.name, cs.c = name, c
    st = cs.st = disjoint_stream(F, k, c["n"], per_field=(0, 2), p_weighted=0.3, p_dup=0.15, seed=c["seed"])
    mi, ocfg, ots = make_pair(F, k, st.bits, st.ffm_bits, opt, interactions=c["inter"], **opt_kwargs(opt))
    layers3 = [(w, a, "hu") for w, a in c["layers"]]
    mi.nn_layers = [dict(width=w, activation=a, init=i) for w, a, i in layers3]
    mi.nn_topology, mi.nn_init_acc_gradient = c["topo"], c["nn_init_acc"]
    cs.mi, cs.ocfg, cs.ots = mi, ocfg, ots
    cs.nn = fwo.make_nn_config(layers3, c["topo"], mi.nn_learning_rate, mi.nn_power_t, mi.nn_init_acc_gradient)
    cfg = cs.cfg = DeepConfig(ocfg, c["layers"], c["topo"], mi.nn_learning_rate, mi.nn_power_t, mi.nn_init_acc_gradient)
    fbt = fw.FeatureBufferTranslator(mi)
    cs.fbs = [fbt.translate(st.recs[int(st.off[e]):int(st.off[e + 1])], e) for e in range(st.n)]
    rng = np.random.default_rng(977 + c["seed"])
    cs.ffm_w, cs.ffm_acc, _ = ffm_ref.warm_state(st)  # (a prefix of the tables that holds every row; the rest keeps its initial values)
    n_lr = 1 << st.bits
    cs.lr = np.empty(2 * n_lr, dtype=np.float32)
    cs.lr[0::2] = rng.uniform(-0.6, 0.6, n_lr) / np.sqrt(st.n_ns)
    cs.lr[1::2] = rng.uniform(1.0, 4.0, n_lr)
    en = Entries([fb.lr_buffer for fb in cs.fbs], [fb.ffm_buffer for fb in cs.fbs])
    x64, _, _ = head_inputs64(cs.lr, cs.ffm_w, cfg.C, F, k, en)
    cs.nn_w = dense_head_weights(x64, c["layers"], c["topo"], seed=c["seed"], z_max=Z_MAX)
    a_init = np.float32(initial_acc(opt, c["nn_init_acc"]))
    base = np.exp(rng.uniform(0.0, np.log(64.0), cfg.total)).astype(np.float32)
    at_init = rng.random(cfg.total) < 0.25
    cs.nn_acc = []
    for e, fb in enumerate(cs.fbs):
        a = np.where(at_init, a_init, base).astype(np.float32)
        if c["nn_init_acc"] == 0.0 and opt != SGD:
            ref = step(cfg, (cs.lr, cs.ffm_w, cs.ffm_acc, cs.nn_w, a), fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance)
            stepped = np.zeros(cfg.total, dtype=bool)
            stepped[ref.nn_idx[ref.nn_dacc != 0.0]] = True
            a = np.where(at_init & stepped, base, a).astype(np.float32)
        cs.nn_acc.append(a)
    _BUILT[name] = cs
    return cs


def vec_form(cfg, threads):
    """per layer (the final neuron last): does nn_layer_backward_any take the 16-byte form?  Its four conditions restated: in % 4 == 0 (in >= 4), the layer's offset
    % 4 == 0, in / 4 <= threads, out <= threads"""
    return [w_in >= 4 and w_in % 4 == 0 and o % 4 == 0 and w_in // 4 <= threads and out <= threads for o, out, w_in in cfg.lay]


def write_oracle(om, cs, e):
    """the case's written state of probe e into an oracle model's own arrays"""
    om.lr_table[:] = cs.lr
    om.ffm_weights[:len(cs.ffm_w)] = cs.ffm_w
    om.ffm_acc[:len(cs.ffm_acc)] = cs.ffm_acc
    o = 0
    for l in range(len(cs.c["layers"]) + 1):
        wv, av = om.nn_weights(l), om.nn_acc(l)
        wv[:] = cs.nn_w[o:o + wv.size]
        av[:] = cs.nn_acc[e][o:o + av.size]
        o += wv.size
    assert o == cs.cfg.total


def read_oracle(om, cs):
    """(LR, FFM_W, FFM_ACC, NN_W, NN_ACC): copies of an oracle model's tables"""
    L = len(cs.c["layers"])
    return (om.lr_table.copy(), om.ffm_weights.copy(), om.ffm_acc.copy(), np.concatenate([om.nn_weights(l).copy() for l in range(L + 1)]),
            np.concatenate([om.nn_acc(l).copy() for l in range(L + 1)]))
