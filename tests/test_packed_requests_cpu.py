"""Context caches and the requests route on packed FFM weights (fwgpu_packed_enable_caches) where no GPU is needed: the packed cache build kernel
restated in numpy in its stated summation order, the regrouped pass on the values the buckets stand for inside ffm_ref.judge_prediction's bound on
every candidate of every shape, and the faults a packed route can have -- caches from the source weights, exchanged half-words in either kernel, the
header of the block before a refresh, and the five faults of requests_cases.FAULTS -- each outside it (tests/packed_requests_cases.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import ffm_ref
import packed_requests_cases as pq
import requests_cases as rq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SHAPES = pytest.mark.parametrize("F,k", pq.SHAPES, ids=[f"{F}x{k}" for F, k in pq.SHAPES])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _failed(view, cands, refs, fault=None):
    n = 0
    for x, ref in zip(cands, refs):
        err, bound, _ = ffm_ref.judge_prediction(rq.emulate(view, x, fault=fault), *ref)
        n += err > bound
    return n


def test_quantiser_restated():
    """the block of a small table by hand: header from the rounded extremes, buckets as f16 numbers, the conversion back exact + one multiply + one add"""
    w = np.array([-0.49996, 0.25, 0.0, 0.49996, 0.1], dtype=np.float32)
    inc, mn, b = pq.quantize(w)
    assert mn == np.float32(-0.5) and inc == np.float32(np.float32(np.float32(0.5) - np.float32(-0.5)) / np.float32(65025.0))
    # 0.00004 / increment = 2.6 -> bucket 3; 0.99996 / increment = 65022.4 -> 65022, which f16 holds as 65024 (numbers above 32768 are 32 apart)
    assert b.dtype == np.uint16 and b.view(np.float16)[0] == np.float16(3.0) and b.view(np.float16)[3] == np.float16(65024.0)
    back = pq.dequantize(inc, mn, b)
    assert np.abs(back - w).max() <= 32 * float(inc)  # (f16 numbers above 32768 are 32 buckets apart)
    assert np.array_equal(pq.swap_halves(np.arange(5, dtype=np.uint16)), np.array([1, 0, 3, 2, 4], dtype=np.uint16))


@pytest.mark.parametrize("F,k", [(6, 4), (30, 16)], ids=["6x4", "30x16"])
def test_quantiser_restatement_is_the_librarys_host_quantiser(F, k):
    """the numpy statements give the bytes of fwgpu_quantize_ffm_weights and the floats of fwgpu_dequantize_ffm_weights on a case's whole table"""
    import struct

    from fwumious_wabbit_amd import persistence as P

    pc = pq.case(F, k)
    blob = P.quantize_ffm_weights(pc.src_w)
    assert blob[:8] == struct.pack("<ff", pc.inc, pc.mn)
    assert blob[8:] == pc.buckets.astype("<u2").tobytes()
    assert np.array_equal(_bits(P.dequantize_ffm_weights(blob, len(pc.src_w))), _bits(pc.w))


def test_butterfly_restated():
    v = np.zeros(64, np.float32)
    v[[3, 4, 40]] = [1.0, 2.0 ** -24, 2.0 ** -24]
    # the two small terms meet first (lanes 4 and 40 -> 8 -> 0 at m = 4: 2^-23) and reach the 1 of lane 3 together at m = 1: 1 + 2^-23, where a
    # sequential sum loses both (1 + 2^-24 ties to 1, twice)
    assert pq.wave_sum(v) == np.float32(1.0) + np.float32(2.0 ** -23)
    assert np.float32(np.float32(np.float32(1.0) + np.float32(2.0 ** -24)) + np.float32(2.0 ** -24)) == np.float32(1.0)
    assert pq.wave_sum(np.ones(64, np.float32)) == np.float32(64.0)


@SHAPES
def test_build_kernel_restated(F, k):
    """T is the sequential float32 sum of requests_cases.Cache bit for bit (the same operations in the same order); dcf, summed in the kernel's own order,
    and the counts agree with the float64 values to the rounding of the few terms they have"""
    pc = pq.case(F, k)
    for (_, ctx_ffm), built in zip(pc.contexts, pc.clean.emu_caches):
        seq = rq.Cache(F, k, pc.w, ctx_ffm)
        assert np.array_equal(_bits(built.T), _bits(seq.T))
        fld = (ctx_ffm["contra_field_index"] // k).astype(np.int64)
        assert np.array_equal(built.cnt, np.bincount(fld, minlength=F))
        exact = np.zeros(F)
        for h, v, f in zip(ctx_ffm["hash"].tolist(), ctx_ffm["value"].astype(np.float64), fld.tolist()):
            own = pc.w[h + f * k:h + (f + 1) * k].astype(np.float64)
            exact[f] += v * v * np.sum(own * own)
        # at most 2 features x k / 4 lanes of 4 squares: 3 + 2 roundings per lane sum, 1 per lane add, log2(16) in the butterfly -- 16 half-ulps bound it amply
        assert np.all(np.abs(built.dcf.astype(np.float64) - exact) <= 8 * np.spacing(np.maximum(exact, 1e-30).astype(np.float32)).astype(np.float64))
        assert np.all(built.dcf[built.cnt == 0] == 0.0) and np.all(built.T.reshape(F, F, k)[:, built.cnt == 0, :] == 0.0)


@SHAPES
def test_the_case_is_decided_by_the_reference(F, k):
    pc = pq.case(F, k)
    assert len(pc.cands) == 96 and len(pc.contexts) == 4 and len(pc.contexts[3][1]) == 0
    p = np.array([x.ref[0] for x in pc.cands])
    M = np.array([x.ref[1] for x in pc.cands])
    print(f"PACKED REQUESTS {F}x{k}: increment {pc.inc!r}, min {pc.mn!r}; p in [{p.min():.3f}, {p.max():.3f}], std {p.std():.3f}, C_P M_p up to {ffm_ref.C_P * M.max():.2e}")
    assert p.std() > 0.05 and ffm_ref.C_P * M.max() < ffm_ref.PRED_CAP
    # quantisation moved the weights: the source table is NOT what the buckets stand for
    assert np.abs(pc.w - pc.src_w).max() > 0.0


@SHAPES
def test_clean_pass_on_bucket_values_meets_the_bar(F, k):
    pc = pq.case(F, k)
    worst = 0.0
    for i, x in enumerate(pc.cands):
        p = rq.emulate(pc.clean, x)
        err, bound, need = ffm_ref.judge_prediction(p, *x.ref)
        worst = max(worst, need)
        assert err <= bound, (i, x.cache, x.request, float(p), x.ref, err, bound, need)
    print(f"PACKED REQUESTS {F}x{k}: the float32 emulation on bucket values needs c_p = {worst:.3e} = {worst / ffm_ref.C_P:.3f} C_P")


@SHAPES
def test_planted_packed_faults_fail_the_judge(F, k):
    pc = pq.case(F, k)
    for fault in pq.PACKED_FAULTS:
        view, refs = pq.planted(pc, fault)
        # (the empty cache holds no sum: a fault of the caches alone cannot move its candidates)
        hit = [i for i, x in enumerate(pc.cands) if not (fault in ("source", "swap_build") and x.cache == 3)]
        failed = _failed(view, [pc.cands[i] for i in hit], [refs[i] for i in hit])
        print(f"PACKED REQUESTS {F}x{k}: fault {fault!r} fails {failed} of {len(hit)} candidates")
        assert failed >= 1, fault


@SHAPES
def test_planted_route_faults_fail_the_judge_on_bucket_values(F, k):
    pc = pq.case(F, k)
    for fault in rq.FAULTS:
        hit = rq.applies(pc, fault)
        if not hit:
            assert fault == "chunk" and pc.R <= 256
            continue
        failed = _failed(pc.clean, hit, [x.ref for x in hit], fault=fault)
        print(f"PACKED REQUESTS {F}x{k}: fault {fault!r} fails {failed} of {len(hit)} candidates")
        assert failed >= 1, fault


def test_packed_context_cache_token_needs_packed_weights():
    """new_fw_predictor_prototype refuses the token on its own before it looks for a model or a device"""
    from fwumious_wabbit_amd import _capi as capi
    from fwumious_wabbit_amd.serving import Predictor

    with pytest.raises(capi.FwgpuError) as e:
        Predictor("fw -i /nonexistent/model.fw -t --foreground --packed_context_cache")
    assert "--packed_context_cache" in e.value.message and "--packed_weights" in e.value.message, e.value


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_packed_kernels_compile_without_spills(tmp_path):
    """every instantiation of the predict kernel and the packed cache build kernel, device only: 0 spilled SGPRs, 0 spilled VGPRs, no scratch"""
    src = os.path.join(ROOT, "fwumious_wabbit_amd", "csrc")
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{src}", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-S", os.path.join(src, "requests.hip"), "-o", str(tmp_path / "requests.s")]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    seen, name = {}, None
    for line in run.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)(?: \[-Rpass)", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            name = t.split(":", 1)[1].strip()
            seen[name] = {}
        elif name and ":" in t:
            key, val = t.rsplit(":", 1)
            seen[name][key.strip()] = val.strip()
    predict = [n for n in seen if "requests_predict_kernel" in n]
    assert len(predict) == 3, sorted(seen)  # f32 at its depth, packed at 4 and at 8 rows in flight
    assert sum("packed_cache_build_kernel" in n for n in seen) == 1, sorted(seen)
    for kn, res in seen.items():
        print(f"PACKED REQUESTS {kn}: {res}")
        assert int(res["SGPRs Spill"]) == 0 and int(res["VGPRs Spill"]) == 0 and int(res["ScratchSize [bytes/lane]"]) == 0, (kn, res)
