"""The requests route (fwgpu_batch_set_caches, csrc/requests.hip) where no GPU is needed: its regrouped forward pass restated in float32 numpy with
strictly sequential sums (tests/requests_cases.py) stays inside ffm_ref.judge_prediction's bound against the float64 pass over the WHOLE request on
every candidate of every shape, five planted faults do not, and both kernels compile for gfx950 without spilling a register."""
import os
import re
import subprocess

import numpy as np
import pytest

import ffm_ref
import requests_cases as rq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SHAPES = pytest.mark.parametrize("F,k", rq.SHAPES, ids=[f"{F}x{k}" for F, k in rq.SHAPES])


@SHAPES
def test_sets_are_what_the_route_is_tested_on(F, k):
    cs = rq.case(F, k)
    assert len(cs.cands) == 96 and [x.cache for x in cs.cands[:8]] == [0, 1, 2, 3, 0, 1, 2, 3]
    for s in cs.sets:
        assert len(s.requests[0].rest) == 0, "request 0 of every set leaves no FFM entry: base + LR"
    assert all(len(x.rest) == len(x.whole) for x in cs.cands if x.cache == 3), "the empty cache filters nothing"
    # the float64 reference alone decides the seeds: the predictions spread and no bound is the cap
    for c in range(3):
        p = np.array([x.ref[0] for x in cs.cands if x.cache == c])
        M = np.array([x.ref[1] for x in cs.cands if x.cache == c])
        print(f"REQUESTS {F}x{k} set {c}: p in [{p.min():.3f}, {p.max():.3f}], std {p.std():.3f}, C_P M_p up to {ffm_ref.C_P * M.max():.2e}")
        assert p.std() > 0.05  # (test_cache_cases_cpu.py's criterion for a set's seed)
        assert ffm_ref.C_P * M.max() < ffm_ref.PRED_CAP


@SHAPES
def test_clean_regrouped_pass_meets_the_bar(F, k):
    cs = rq.case(F, k)
    worst = 0.0
    for i, x in enumerate(cs.cands):
        p = rq.emulate(cs, x)
        err, bound, need = ffm_ref.judge_prediction(p, *x.ref)
        worst = max(worst, need)
        assert err <= bound, (i, x.cache, x.request, float(p), x.ref, err, bound, need)
    print(f"REQUESTS {F}x{k}: the float32 emulation needs c_p = {worst:.3e} = {worst / ffm_ref.C_P:.3f} C_P")


@SHAPES
def test_planted_faults_fail_the_judge(F, k):
    cs = rq.case(F, k)
    for fault in rq.FAULTS:
        hit = rq.applies(cs, fault)
        if not hit:
            assert fault == "chunk" and cs.R <= 256
            continue
        failed = 0
        for x in hit:
            err, bound, _ = ffm_ref.judge_prediction(rq.emulate(cs, x, fault=fault), *x.ref)
            failed += err > bound
        print(f"REQUESTS {F}x{k}: fault {fault!r} fails {failed} of {len(hit)} candidates")
        assert failed >= 1, fault


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernels_compile_without_spills(tmp_path):
    """both kernels of requests.hip, device only: 0 spilled SGPRs, 0 spilled VGPRs, no scratch (the remarks scripts/hot_probe.py reads)"""
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
            name = next((kn for kn in ("requests_base_kernel", "requests_predict_kernel") if kn in t), None)
            if name:
                seen[name] = {}
        elif name and ":" in t:
            key, val = t.rsplit(":", 1)
            seen[name][key.strip()] = val.strip()
    assert set(seen) == {"requests_base_kernel", "requests_predict_kernel"}, run.stderr[-2000:]
    for kn, res in seen.items():
        print(f"REQUESTS {kn}: {res}")
        assert int(res["SGPRs Spill"]) == 0 and int(res["VGPRs Spill"]) == 0 and int(res["ScratchSize [bytes/lane]"]) == 0, (kn, res)
