"""A float64 restatement of the deep head's predict-only forward, for the tests of the batched head predict route
(test_head_predict_ref_cpu.py pins it against the oracle on the CPU; test_gpu_head_predict.py judges the device with it), and of one
training step of the mini-batched head (head_train64: test_head_train_ref_cpu.py pins it against the oracle's micro-batch mode,
test_gpu_head_train.py judges the kernels of head.hip with it).

Both rules of the head input come from oracle/fw_oracle.c, not from the kernels:
  * slot c < C: lr_forward -- the sum of w[hash] * value over the LR entries of combo c;
  * slot C + t, t = i (i + 1) / 2 + j for j <= i: fwo_triangle_forward over the FFM block's F x F outputs -- for j < i twice the
    half pair product, i.e. sum_kk S_i[j, kk] * S_j[i, kk] with S_f the value-weighted sum of field f's rows (ffm_forward); on the
    diagonal the per-feature form of ffm_fb_forward: sum over the field's features a of 0.5 * sum_kk (w_a v_a) (S_f[f, kk] - w_a v_a),
    which is EXACTLY 0 for a field of at most one feature.
Everything is plain numpy in float64, vectorised over the examples of a batch."""
import numpy as np

import fwumious_wabbit_amd as fw
from helpers import make_pair
from oracle import fwo

PRED_TOL = 1e-5      # the project's bars (test_gpu_parity.py)
LOGLOSS_TOL = 1e-4

# The shapes of the batched-route tests: n_ns namespaces == fields, k, namespace-pair interactions, hidden layers (width, activation), topology.
# X = (n_ns + interactions + 1 constant) + F (F + 1) / 2.
SHAPES = {
    "a": dict(F=6, k=4, inter=[(0, 1)], layers=[(12, "relu"), (8, "relu")], topo="one"),       # X = 29: X % 4 != 0, single-chunk rows
    "b": dict(F=30, k=8, inter=[], layers=[(64, "relu"), (64, "relu")], topo="one"),            # R = 240, X = 496
    "c": dict(F=30, k=16, inter=[], layers=[(256, "relu"), (256, "relu")], topo="one"),         # config E: R = 480, two-chunk rows
    "d": dict(F=5, k=4, inter=[], layers=[(9, "none"), (7, "relu")], topo="two"),               # identity layer, topology two
    "e": dict(F=20, k=12, inter=[], layers=[(16, "relu")], topo="one"),                         # k not a power of two, R = 240
    "f": dict(F=22, k=12, inter=[], layers=[(16, "relu")], topo="one"),                         # R = 264 and 256 % 12 != 0: the gate refuses
    "g256": dict(F=32, k=8, inter=[], layers=[(16, "relu")], topo="one"),                       # R = 256: the last single-chunk shape
    "g260": dict(F=65, k=4, inter=[], layers=[(16, "relu")], topo="one"),                       # R = 260: the first two-chunk shape, NT = 2145
    "h": dict(F=4, k=4, inter=[], layers=[(8, "relu")], topo="one"),
}


# Further heads for the tests of the training step, on shape a's inputs (X = 29): one unit; widths below, at and above the 64-column tiles, the width
# being the K of the second layer's forward product and of the first layer's input-gradient product
TRAIN_SHAPES = {
    "w1": dict(F=6, k=4, inter=[(0, 1)], layers=[(1, "relu")], topo="one"),
    "w63": dict(F=6, k=4, inter=[(0, 1)], layers=[(63, "relu"), (63, "relu")], topo="one"),
    "w64": dict(F=6, k=4, inter=[(0, 1)], layers=[(64, "relu"), (64, "relu")], topo="one"),
    "w65": dict(F=6, k=4, inter=[(0, 1)], layers=[(65, "relu"), (65, "relu")], topo="one"),
}


def shape_of(name):
    """(X, layers, topo) of a shape of SHAPES / TRAIN_SHAPES"""
    s = SHAPES.get(name) or TRAIN_SHAPES[name]
    F = s["F"]
    return F + len(s["inter"]) + 1 + F * (F + 1) // 2, s["layers"], s["topo"]


def build_shape(name, bits=14, optimizer=fw.Optimizer.AdagradLUT):
    """(ModelInstance with the head, oracle config, oracle translator, oracle nn config) of SHAPES[name]"""
    s = SHAPES.get(name) or TRAIN_SHAPES[name]
    mi, ocfg, ots = make_pair(s["F"], s["k"], bits, bits, optimizer, interactions=s["inter"])
    layers = [(w, a, "hu") for w, a in s["layers"]]
    mi.nn_layers = [dict(width=w, activation=a, init=i) for w, a, i in layers]
    mi.nn_topology = s["topo"]
    nn = fwo.make_nn_config(layers, s["topo"], mi.nn_learning_rate, mi.nn_power_t, mi.nn_init_acc_gradient)
    return mi, ocfg, ots, nn


def stream(name, n, seed, first=0):
    """the synthetic records of a shape: about one extra feature per namespace, a tenth of them weighted"""
    return fw.synth_records(SHAPES[name]["F"], 1.0, 1.1, 3000, 0.1, seed, first, n)


class Entries:
    """the translated entries of a batch, flat: lr / ffm (the structured arrays of the translator) with the example of each entry"""

    def __init__(self, lrs, ffms):
        self.n = len(lrs)
        self.lr = np.concatenate(lrs) if lrs else np.zeros(0, fwo.LR_ENTRY)
        self.ffm = np.concatenate(ffms) if ffms else np.zeros(0, fwo.FFM_ENTRY)
        self.lr_ex = np.repeat(np.arange(self.n), [len(x) for x in lrs])
        self.ffm_ex = np.repeat(np.arange(self.n), [len(x) for x in ffms])
        self.lrs, self.ffms = lrs, ffms


def translate(ots, recs, off, which=None):
    """Entries of the records `which` (default: all) through the oracle's translator"""
    lrs, ffms = [], []
    for e in (range(len(off) - 1) if which is None else which):
        lr, ffm, _, _ = ots.translate(recs[int(off[e]):int(off[e + 1])], cap=1024)
        lrs.append(lr), ffms.append(ffm)
    return Entries(lrs, ffms)


def head_inputs64(lr_table, ffm_w, C, F, k, en, chunk=256):
    """x64 [n, X], sum_abs [n, X] (the float64 sum of the absolute products that make up each slot) and exact0 [n, X] (slots the reference
    defines as exactly 0: a combo with no entry, the diagonal of a field with at most one feature).
    lr_table: the interleaved {w, acc} LR table; ffm_w: the FFM weight table (as table_read / the oracle's views give them)."""
    n = en.n
    NT = F * (F + 1) // 2
    X = C + NT
    x, sa = np.zeros((n, X)), np.zeros((n, X))
    exact0 = np.zeros((n, X), dtype=bool)
    w_lr = np.asarray(lr_table, dtype=np.float64)[0::2]
    prod = w_lr[en.lr["hash"].astype(np.int64)] * en.lr["value"].astype(np.float64)
    combo = en.lr["combo_index"].astype(np.int64)
    np.add.at(x, (en.lr_ex, combo), prod)
    np.add.at(sa, (en.lr_ex, combo), np.abs(prod))
    cnt = np.zeros((n, C), dtype=np.int64)
    np.add.at(cnt, (en.lr_ex, combo), 1)
    exact0[:, :C] = cnt == 0
    if not F:
        return x, sa, exact0
    R = F * k
    W = np.asarray(ffm_w, dtype=np.float64)
    fld = (en.ffm["contra_field_index"] // k).astype(np.int64)
    order = np.argsort(en.ffm_ex * F + fld, kind="stable")  # (the translator's order already: by example, by field)
    ex_s, fld_s = en.ffm_ex[order], fld[order]
    h_s, v_s = en.ffm["hash"].astype(np.int64)[order], en.ffm["value"].astype(np.float64)[order]
    nf = np.zeros((n, F), dtype=np.int64)
    np.add.at(nf, (ex_s, fld_s), 1)
    ii, jj = np.tril_indices(F)  # t = i (i + 1) / 2 + j, j <= i: fwo_triangle_forward's order
    diag = ii == jj
    exact0[:, C:][:, diag] = nf <= 1
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        a, b = np.searchsorted(ex_s, lo), np.searchsorted(ex_s, hi)
        S = np.zeros((hi - lo, F, R))
        Sa = np.zeros((hi - lo, F, R))
        D = np.zeros((hi - lo, F))
        Da = np.zeros((hi - lo, F))
        if b > a:
            rows = W[h_s[a:b, None] + np.arange(R)[None, :]] * v_s[a:b, None]  # every feature's row times its value
            key = (ex_s[a:b] - lo) * F + fld_s[a:b]
            starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
            ke, kf = key[starts] // F, key[starts] % F
            S[ke, kf] = np.add.reduceat(rows, starts, axis=0)
            Sa[ke, kf] = np.add.reduceat(np.abs(rows), starts, axis=0)
            # the diagonal, per feature: 0.5 * sum_kk (w v) * (S_f[f] - w v)
            m = b - a
            own = rows.reshape(m, F, k)[np.arange(m), fld_s[a:b]]
            S_own = S.reshape(hi - lo, F, F, k)[ex_s[a:b] - lo, fld_s[a:b], fld_s[a:b]]
            Sa_own = Sa.reshape(hi - lo, F, F, k)[ex_s[a:b] - lo, fld_s[a:b], fld_s[a:b]]
            np.add.at(D, (ex_s[a:b] - lo, fld_s[a:b]), 0.5 * (own * (S_own - own)).sum(axis=1))
            np.add.at(Da, (ex_s[a:b] - lo, fld_s[a:b]), 0.5 * (np.abs(own) * (Sa_own - np.abs(own))).sum(axis=1))
        S4, Sa4 = S.reshape(hi - lo, F, F, k), Sa.reshape(hi - lo, F, F, k)
        P = (S4 * S4.transpose(0, 2, 1, 3)).sum(axis=3)
        Pa = (Sa4 * Sa4.transpose(0, 2, 1, 3)).sum(axis=3)
        tri, tri_a = P[:, ii, jj], Pa[:, ii, jj]
        tri[:, diag], tri_a[:, diag] = D, Da
        tri[:, diag] = np.where(nf[lo:hi] <= 1, 0.0, tri[:, diag])
        x[lo:hi, C:], sa[lo:hi, C:] = tri, tri_a
    return x, sa, exact0


def head_layout(X, layers, topo):
    """[(offset, out, in)] of every layer of the TABLE_NN_W blob, the final neuron last: per layer `out x in` weights (row per neuron), then `out` biases
    (test_deep_head_blob_round_trip_and_inference); the final neuron reads [h_last | x] in topology one, h_last alone in topology two"""
    lay, o, w_in = [], 0, X
    for w, _ in layers:
        lay.append((o, w, w_in))
        o += (w_in + 1) * w
        w_in = w
    fin = w_in + (X if topo == "one" else 0)
    lay.append((o, 1, fin))
    return lay, o + fin + 1


def head_forward64(x, nn_w, layers, topo):
    """(p64, z64) of the head over x [n, X]: hidden layers z = W h + b with ReLU or identity, the final neuron, then the sigmoid's rules
    (sigmoid_block: NaN -> logistic(0), beyond +-50 -> logistic(+-50))"""
    nn_w = np.asarray(nn_w, dtype=np.float64)
    lay, total = head_layout(x.shape[1], layers, topo)
    assert nn_w.size == total
    h = x
    for (o, out, w_in), (_, act) in zip(lay[:-1], layers):
        Wl = nn_w[o:o + out * w_in].reshape(out, w_in)
        h = h @ Wl.T + nn_w[o + out * w_in:o + out * w_in + out]
        if act == "relu":
            h = np.where(h < 0.0, 0.0, h)
    o, _, fin = lay[-1]
    fx = np.concatenate([h, x], axis=1) if topo == "one" else h
    with np.errstate(invalid="ignore", over="ignore"):
        z = fx @ nn_w[o:o + fin] + nn_w[o + fin]
        zc = np.where(np.isnan(z), 0.0, np.clip(z, -50.0, 50.0))
        p = 1.0 / (1.0 + np.exp(-zc))
    return p, z


# One dot product of f32 terms summed in any order, against the same sum in float64: |got - want| <= DOT_REL * sum |a||b| + DOT_ABS
# (the project's number: test_head_products_match_a_torch_f32_reference)
DOT_REL, DOT_ABS = 2e-5, 1e-6


def dot_bound(sum_abs):
    return DOT_REL * np.asarray(sum_abs, dtype=np.float64) + DOT_ABS


def head_train64(x, yi, nn_w, layers, topo):
    """One training step of the mini-batched head in float64, by the rules of oracle/fw_oracle.c (fwo_learn_minibatch, sigmoid_block): every example
    against the same dense weights, the weight gradients summed over the batch.  x [n, X], yi [n, 2] = {label, importance}.
      * a ReLU unit's mask is 0 where pre < 0 and 1 elsewhere (pre >= 0; a NaN passes, as in the oracle); an identity layer's mask is all ones;
      * g = -(label - p) * importance; 0 for importance 0, for a NaN logit and beyond +-50;
      * an example with g == 0 contributes exactly nothing to dW and has dx == 0 -- whatever its x holds, inf and NaN included;
      * topology one adds the direct g * w_f[wl:] into dx.
    Returns a dict of float64 arrays: pre / h / mask / dz (lists, one [n, out_l] array per hidden layer), z, p, g [n], dx [n, X] and dW in
    TABLE_NN_W layout (head_layout); under "sa" the same keys hold, for each element, the sum of the absolute products that formed it in ITS OWN
    stage (for a stage-wise bound: dot_bound(sa)); under "tol" the bound propagated from x through every stage before it, each stage adding
    dot_bound of its own sums to what its inputs carry (for a whole-chain comparison on the host inputs alone; it holds where the masks agree)."""
    x = np.asarray(x, dtype=np.float64)
    yi = np.asarray(yi, dtype=np.float64).reshape(-1, 2)
    nn_w = np.asarray(nn_w, dtype=np.float64)
    n, X = x.shape
    lay, total = head_layout(X, layers, topo)
    assert nn_w.size == total and len(yi) == n
    L = len(layers)
    Ws = [nn_w[o:o + out * w_in].reshape(out, w_in) for o, out, w_in in lay]
    bs = [nn_w[o + out * w_in:o + out * w_in + out] for o, out, w_in in lay]
    ulp = 2.0 ** -23
    with np.errstate(invalid="ignore", over="ignore"):
        pre, h, mask, sa_pre, t_h = [], [], [], [], []
        hin, t_in = x, np.zeros_like(x)
        for l in range(L):
            z_l = hin @ Ws[l].T + bs[l]
            s_l = np.abs(hin) @ np.abs(Ws[l]).T + np.abs(bs[l])
            m_l = np.where(z_l < 0.0, 0.0, 1.0) if layers[l][1] == "relu" else np.ones_like(z_l)
            e_l = (dot_bound(s_l) + t_in @ np.abs(Ws[l]).T) * m_l
            pre.append(z_l), sa_pre.append(s_l), mask.append(m_l), t_h.append(e_l)
            h.append(np.where(m_l == 0.0, 0.0, z_l))
            hin, t_in = h[-1], e_l
        wl = lay[-2][1]
        wf, bf = Ws[L][0], bs[L][0]
        fx = np.concatenate([hin, x], axis=1) if topo == "one" else hin
        t_fx = np.concatenate([t_in, np.zeros_like(x)], axis=1) if topo == "one" else t_in
        z = fx @ wf + bf
        sa_z = np.abs(fx) @ np.abs(wf) + abs(bf)
        t_z = dot_bound(sa_z) + t_fx @ np.abs(wf)
        sat = np.isnan(z) | (np.abs(z) > 50.0)
        zc = np.where(np.isnan(z), 0.0, np.clip(z, -50.0, 50.0))
        p = 1.0 / (1.0 + np.exp(-zc))
        label, imp = yi[:, 0], yi[:, 1]
        g = np.where(sat | (imp == 0.0), 0.0, -(label - p) * imp)
        t_p = 0.25 * t_z + ulp
        t_g = np.abs(imp) * t_p + ulp * np.abs(g)
    on = np.flatnonzero(g != 0.0)  # the other examples are left out of every product below: exactly nothing, whatever their rows hold
    assert np.all(np.isfinite(x[on])), "a finite logit inside +-50 from a non-finite x"
    go, t_go = g[on], t_g[on]
    dW, sa_dW, t_dW = np.zeros(total), np.zeros(total), np.zeros(total)
    dz, sa_dz, t_dz = [None] * L, [None] * L, [None] * L
    dx, sa_dx, t_dx = np.zeros((n, X)), np.zeros((n, X)), np.zeros((n, X))

    def rows(full, part, width):
        out = np.zeros((n, width))
        out[on] = part
        return out

    # final neuron: dW_f = sum_e g_e [h_last | x]_e, its bias sum_e g_e; d h_last = g w_f[:wl] through the last mask; the direct part of dx
    o, _, fin = lay[L]
    fxo, t_fxo = fx[on], t_fx[on]
    dW[o:o + fin] = go @ fxo
    sa_dW[o:o + fin] = np.abs(go) @ np.abs(fxo)
    t_dW[o:o + fin] = dot_bound(sa_dW[o:o + fin]) + t_go @ np.abs(fxo) + np.abs(go) @ t_fxo
    dW[o + fin], sa_dW[o + fin] = go.sum(), np.abs(go).sum()
    t_dW[o + fin] = dot_bound(sa_dW[o + fin]) + t_go.sum()
    d = go[:, None] * wf[None, :wl] * mask[L - 1][on]
    t_d = (t_go[:, None] * np.abs(wf[None, :wl]) + 2 * ulp * np.abs(go[:, None] * wf[None, :wl])) * mask[L - 1][on]
    direct = go[:, None] * wf[None, wl:] if topo == "one" else np.zeros((len(on), X))
    t_direct = t_go[:, None] * np.abs(wf[None, wl:]) + ulp * np.abs(direct) if topo == "one" else np.zeros((len(on), X))
    s_d = np.abs(d)
    for l in range(L - 1, -1, -1):
        dz[l], sa_dz[l], t_dz[l] = rows(n, d, lay[l][1]), rows(n, s_d, lay[l][1]), rows(n, t_d, lay[l][1])
        o, out, w_in = lay[l]
        lin = (x if l == 0 else h[l - 1])[on]
        t_lin = (np.zeros_like(x) if l == 0 else t_h[l - 1])[on]
        blk = slice(o, o + out * w_in)
        sa_blk = np.abs(d).T @ np.abs(lin)
        dW[blk], sa_dW[blk] = (d.T @ lin).reshape(-1), sa_blk.reshape(-1)
        t_dW[blk] = (dot_bound(sa_blk) + t_d.T @ np.abs(lin) + np.abs(d).T @ t_lin).reshape(-1)
        bb = slice(o + out * w_in, o + out * w_in + out)
        dW[bb], sa_dW[bb] = d.sum(axis=0), np.abs(d).sum(axis=0)
        t_dW[bb] = dot_bound(sa_dW[bb]) + t_d.sum(axis=0)
        din, s_in = d @ Ws[l], np.abs(d) @ np.abs(Ws[l])
        t_din = dot_bound(s_in) + t_d @ np.abs(Ws[l])
        if l > 0:
            d, s_d, t_d = din * mask[l - 1][on], s_in * mask[l - 1][on], t_din * mask[l - 1][on]
        else:
            dx[on], sa_dx[on], t_dx[on] = direct + din, np.abs(direct) + s_in, t_direct + t_din + ulp * np.abs(direct + din)
    return dict(pre=pre, h=h, mask=mask, z=z, p=p, g=g, dz=dz, dx=dx, dW=dW,
                sa=dict(pre=sa_pre, h=sa_pre, z=sa_z, dz=sa_dz, dx=sa_dx, dW=sa_dW),
                tol=dict(h=t_h, z=t_z, p=t_p, g=t_g, dz=t_dz, dx=t_dx, dW=t_dW))


RELU_MARGIN = 4.0  # a drawn example is kept if every ReLU unit's |pre64| is above this many forward bounds of its layer


def draw_train_case(name, n, seed, conc=0.0):
    """A seeded batch for one training step of the head of shape `name`, drawn on the host: x = N(0, 1) times a per-slot scale (log-normal), labels 0 / 1,
    importances 1 / 0.5 / 0 mixed (example e: 0.5 where e % 5 == 3, 0 where e % 7 == 5), dense weights in which every slot of x and every unit matters:
    first-layer column i and the final neuron's direct weight on x_i are N(0, 1) / (slot scale * sqrt(in)), the other weights N(0, 1) / sqrt(in), biases
    N(0, 0.5); the final neuron is then scaled so that the largest |logit| over all drawn examples is 4.  `conc` > 0 gives the columns of every
    layer log-normal importances (sigma = conc, normalised): fewer terms dominate a unit's sum, so that a wide layer's pre-activations are less often
    within rounding of 0 (K terms of random sign: sum |products| / |sum| grows like sqrt(K)).
    Examples with a ReLU unit whose |pre64| <= RELU_MARGIN * dot_bound(its sum of absolute products) are rejected -- by the reference alone -- until n
    are kept: f32 and float64 may legitimately disagree about such a unit's mask.  Returns dict(x, yi, w: float32; ref: head_train64 of exactly these
    float32 values; drawn, rejected: examples looked at / rejected among them)."""
    X, layers, topo = shape_of(name)
    rng = np.random.default_rng(seed)
    slot = np.exp(rng.normal(0.0, 1.0, X))
    pool = n + n // 4 + 32
    xs = (rng.standard_normal((pool, X)) * slot).astype(np.float32)
    lay, total = head_layout(X, layers, topo)
    w = np.zeros(total)
    for li, (o, out, w_in) in enumerate(lay):
        imp = np.exp(rng.normal(0.0, conc, w_in)) if conc else np.ones(w_in)
        imp *= np.sqrt(w_in / (imp ** 2).sum())
        Wl = rng.standard_normal((out, w_in)) * imp / np.sqrt(w_in)
        if li == 0:
            Wl /= slot
        elif li == len(lay) - 1 and topo == "one":
            Wl[0, w_in - X:] /= slot
        w[o:o + out * w_in] = Wl.reshape(-1)
        w[o + out * w_in:o + out * w_in + out] = 0.5 * rng.standard_normal(out)
    _, z = head_forward64(xs.astype(np.float64), w, layers, topo)
    o, _, fin = lay[-1]
    w[o:o + fin + 1] *= 3.999 / np.abs(z).max()  # (inside 4 after the rounding to float32 too)
    w = w.astype(np.float32)
    yi_all = np.stack([rng.integers(0, 2, pool), np.ones(pool)], axis=1).astype(np.float32)
    ref = head_train64(xs, yi_all, w, layers, topo)
    near = np.zeros(pool, dtype=bool)
    for l, (_, act) in enumerate(layers):
        if act == "relu":
            near |= (np.abs(ref["pre"][l]) <= RELU_MARGIN * dot_bound(ref["sa"]["pre"][l])).any(axis=1)
    kept = np.flatnonzero(~near)[:n]
    assert len(kept) == n, "the pool is too small"
    drawn = int(kept[-1]) + 1
    x, yi = xs[kept], yi_all[kept]
    e = np.arange(n)
    yi[e % 5 == 3, 1] = 0.5
    yi[e % 7 == 5, 1] = 0.0
    ref = head_train64(x, yi, w, layers, topo)
    assert np.abs(ref["z"]).max() <= 4.0
    return dict(x=x, yi=yi, w=w, ref=ref, drawn=drawn, rejected=drawn - n, layers=layers, topo=topo, X=X)


# The batches of test_gpu_head_train.py: (shape, n, seed, conc).  n around the 16 row groups of the column sums, around the 64-row tiles, ragged; on config
# E's geometry ("c": 193 777 dense weights, beyond one trip of the optimizer step's grid) 64 and 72 take the split-K gradient product, 100 the tiled one.
# test_head_train_ref_cpu.py checks that every one of them rejects fewer than a tenth of its draws.
_NS = (1, 15, 16, 17, 63, 64, 65, 72, 100, 128)
TRAIN_CASES = ([("a", n, 1000 + n, 0.0) for n in _NS] + [("w65", n, (2315 if n == 15 else 2000 + n), 0.0) for n in _NS] +
               [("d", 72, 3072, 0.0), ("w1", 72, 4072, 0.0), ("w63", 72, 5063, 0.0), ("w64", 72, 5064, 0.0),
                ("c", 64, 6064, 3.0), ("c", 72, 6072, 3.0), ("c", 100, 6100, 3.0)])
REGROW_CASES = [("a", 16, 1016, 0.0), ("a", 128, 1128, 0.0), ("a", 17, 1017, 0.0)]  # one regressor: the scratch buffers grow, then serve a smaller batch
MAX_REJECTED = 0.1


def dense_head_weights(x64, layers, topo, seed, z_max=4.0):
    """Dense head weights that make every slot of x matter: column i of the first layer and the final neuron's direct weight on x_i are N(0, 1) draws
    divided by the largest |x_i| of the stream (1 where the slot is always 0) and by sqrt(X), so every slot moves the logit by a comparable amount; the
    other layers are N(0, 1) / sqrt(in), biases N(0, 0.1).  The final neuron is then scaled so that the largest |logit| of the stream is z_max: far
    inside (-20, 20), where the sigmoid still has a slope that shows an error of the logit in the prediction."""
    rng = np.random.default_rng(seed)
    X = x64.shape[1]
    scale = np.abs(x64).max(axis=0)
    scale[scale == 0.0] = 1.0
    lay, total = head_layout(X, layers, topo)
    w = np.zeros(total)
    for li, (o, out, w_in) in enumerate(lay):
        Wl = rng.standard_normal((out, w_in)) / np.sqrt(w_in)
        if li == 0:
            Wl = rng.standard_normal((out, X)) / (scale[None, :] * np.sqrt(X))
        elif li == len(lay) - 1 and topo == "one":
            Wl[0, w_in - X:] = rng.standard_normal(X) / (scale * np.sqrt(w_in))
        w[o:o + out * w_in] = Wl.reshape(-1)
        w[o + out * w_in:o + out * w_in + out] = 0.1 * rng.standard_normal(out)
    _, z = head_forward64(x64, w, layers, topo)
    o, _, fin = lay[-1]
    w[o:o + fin + 1] *= z_max / np.abs(z).max()
    return w.astype(np.float32)


def mirror_into_oracle(om, lr_table, ffm_w, nn_w, n_layers):
    """the given tables into an oracle model's own arrays (its views are writable)"""
    om.lr_table[:] = lr_table
    if len(ffm_w):
        om.ffm_weights[:] = ffm_w
    o = 0
    for l in range(n_layers + 1):
        v = om.nn_weights(l)
        v[:] = nn_w[o:o + v.size]
        o += v.size
    assert o == len(nn_w)


def logits_of(p):
    p = np.asarray(p, dtype=np.float64)
    return np.log(p) - np.log1p(-p)


# ------------------------------------------------------------------ entry batches built by hand
CRAFTED_KINDS = ("lr_out_of_combo_order", "duplicate_lr_hashes", "a_combo_without_entry", "no_lr_entries", "no_ffm_features",
                 "every_field_one_feature", "a_field_with_the_same_feature_twice", "a_field_with_two_features", "weighted_features",
                 "importance_0_or_half")


def crafted_examples(pool_lr, pool_ffm, C, F, k, n, seed):
    """n examples cycling through CRAFTED_KINDS: [(lr rows, ffm rows, label, importance)], rows as (hash, value, combo_index) and
    (hash, value, contra_field_index), the FFM rows ordered by field as the translator emits them.  Hashes come from the given pools
    (entries a training stream touched, so their weights are not at init)."""
    rng = np.random.default_rng(seed)
    out = []
    for e in range(n):
        kind = CRAFTED_KINDS[e % len(CRAFTED_KINDS)]
        lr = [(int(rng.choice(pool_lr)), 1.0, c) for c in range(C)]
        per_field = [int(rng.integers(0, 3)) for _ in range(F)]
        label, imp = float(e & 1), 1.0
        if kind == "every_field_one_feature":
            per_field = [1] * F
        ffm = [[(int(rng.choice(pool_ffm)), 1.0, f * k) for _ in range(per_field[f])] for f in range(F)]
        if kind == "lr_out_of_combo_order":
            lr = lr[::-1] + [(int(rng.choice(pool_lr)), 0.5, 1)]
        elif kind == "duplicate_lr_hashes":
            lr = lr + [lr[2], (lr[2][0], 2.0, 4)]
            lr.sort(key=lambda r: r[2])
        elif kind == "a_combo_without_entry":
            lr = [r for r in lr if r[2] != 3]
        elif kind == "no_lr_entries":
            lr = []
        elif kind == "no_ffm_features":
            ffm = [[] for _ in range(F)]
        elif kind == "a_field_with_the_same_feature_twice":
            h = int(rng.choice(pool_ffm))
            ffm[2] = [(h, 1.0, 2 * k), (h, 1.0, 2 * k)]
        elif kind == "a_field_with_two_features":
            h1, h2 = (int(v) for v in rng.choice(pool_ffm, size=2, replace=False))
            ffm[2] = [(h1, 1.0, 2 * k), (h2, 1.0, 2 * k)]
        elif kind == "weighted_features":
            lr = [(h, float(rng.choice([0.5, 2.0, -1.5])), c) for h, _, c in lr]
            ffm = [[(h, float(rng.choice([0.5, 2.0, 0.75])), c) for h, _, c in fl] or [(int(rng.choice(pool_ffm)), 1.5, f * k)]
                   for f, fl in enumerate(ffm)]
        elif kind == "importance_0_or_half":
            imp = 0.0 if (e // len(CRAFTED_KINDS)) & 1 else 0.5
        out.append((lr, [r for fl in ffm for r in fl], label, imp))
    return out


def crafted_entries(examples):
    return Entries([fwo.lr_entries(lr) for lr, _, _, _ in examples], [fwo.ffm_entries(ffm) for _, ffm, _, _ in examples])
