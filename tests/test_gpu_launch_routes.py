"""What fwgpu_debug_last_route / fwgpu_debug_last_launch read after the EARLY RETURNS of the batch dispatcher (csrc/launch.cpp run_batch over
pick_route): empty batches, refused updating launches with and without a cache set, and the debug kernel version across a packed launch.

The success path of every route is pinned where the route is tested; here the smallest model that reaches the early returns -- the 6 x 4 case of
requests_cases / packed_requests_cases (tables, four caches, a packed twin), eight candidates per launch.  No expectation is a measured number."""
import numpy as np
import pytest

import cache_cases as cc
import fwumious_wabbit_amd as fw
import packed_requests_cases as pq
import requests_cases as rq
from fwumious_wabbit_amd import _capi as capi

pytestmark = pytest.mark.gpu

TABLES = (capi.TABLE_FFM_W, capi.TABLE_FFM_ACC, capi.TABLE_LR)
N = 8


def _fb(lr, ffm):
    return fw.FeatureBuffer(label=0.0, example_importance=1.0, example_number=0, lr_buffer=lr, ffm_buffer=ffm)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _launch(re, b, update=False):
    re.learn_batch(b, capi.MODE_HOGWILD, update)
    return b.predictions().copy()


def _refused(fn, code=capi.ERR_INVALID):
    with pytest.raises(capi.FwgpuError) as e:
        fn()
    assert e.value.code == code, e.value
    return e.value.message


class _Twins:
    """the f32 regressor on the case's tables with its four caches, its packed twin as it is loaded (no caches) and a second twin with caches enabled"""

    def __init__(self):
        pc = pq.case(6, 4)
        assert pc.rs is rq.case(6, 4).rs
        self.pc = pc
        self.cands = pc.cands[:N]
        self.idx = np.array([x.cache for x in self.cands], dtype=np.uint32)
        self.fbs = [_fb(x.lr, x.rest) for x in self.cands]
        self.f32 = fw.Regressor(cc.models(pc.rs))
        for t, v in zip(TABLES, (pc.src_w, pc.acc, pc.lr)):
            self.f32.table_write(t, v)
        self.packed = self.f32.pack()
        self.cached = self.f32.pack()
        self.cached.enable_packed_caches()
        self.closing = []
        self.f32_caches = [self.f32.setup_cache(_fb(lr, ffm)) for lr, ffm in pc.contexts]
        self.cached_caches = [self.cached.setup_cache(_fb(lr, ffm)) for lr, ffm in pc.contexts]

    def batch(self, re, fbs=None):
        b = re.batch(self.fbs if fbs is None else fbs)
        self.closing.append(b)
        return b

    def close(self):
        for x in self.closing + self.f32_caches + self.cached_caches + [self.packed, self.cached, self.f32]:
            x.close()


@pytest.fixture(scope="module")
def twins():
    t = _Twins()
    yield t
    t.close()


def test_f32_empty_batch_is_route_none_and_leaves_the_last_launch(twins):
    re = twins.f32
    _launch(re, twins.batch(re))
    assert re.last_route() == capi.ROUTE_FUSED
    left = re.last_launch()
    assert left["family"] == capi.KERNEL_RESIDENT, left
    empty = twins.batch(re, [])
    re.learn_batch(empty, capi.MODE_HOGWILD, True)  # (as tests/test_gpu_parity.py sends it)
    assert len(empty.predictions()) == 0
    assert re.last_route() == capi.ROUTE_NONE
    assert re.last_launch() == left
    re.learn_batch(empty, capi.MODE_SEQUENTIAL, False)
    assert re.last_route() == capi.ROUTE_NONE and re.last_launch() == left


def test_packed_empty_batch_is_route_packed(twins):
    for re in (twins.packed, twins.cached):
        _launch(re, twins.batch(re))
        left = re.last_launch()
        assert left["family"] == capi.KERNEL_PACKED, left
        empty = twins.batch(re, [])
        re.learn_batch(empty, capi.MODE_HOGWILD, False)
        assert len(empty.predictions()) == 0
        assert re.last_route() == capi.ROUTE_PACKED
        assert re.last_launch() == left


def test_packed_updating_launch_is_refused_on_route_packed(twins):
    re = twins.packed
    b = twins.batch(re)
    before = _launch(re, b)
    assert re.last_route() == capi.ROUTE_PACKED
    assert "packed" in _refused(lambda: re.learn_batch(b, capi.MODE_HOGWILD, True))
    assert re.last_route() == capi.ROUTE_PACKED
    assert np.array_equal(_bits(_launch(re, b)), _bits(before)) and re.last_route() == capi.ROUTE_PACKED


def test_f32_updating_launch_with_a_set_is_refused_on_route_requests(twins):
    re = twins.f32
    b = twins.batch(re)
    b.set_caches(twins.f32_caches, twins.idx)
    before = _launch(re, b)
    assert re.last_route() == capi.ROUTE_REQUESTS and re.last_launch()["family"] == capi.KERNEL_REQUESTS
    plain = twins.batch(re)
    _launch(re, plain)
    assert re.last_route() == capi.ROUTE_FUSED  # (so that the route below is the refused launch's own)
    assert "predict-only" in _refused(lambda: re.learn_batch(b, capi.MODE_HOGWILD, True))
    assert re.last_route() == capi.ROUTE_REQUESTS
    # the set is still attached
    assert np.array_equal(_bits(_launch(re, b)), _bits(before)) and re.last_route() == capi.ROUTE_REQUESTS


def test_packed_updating_launch_with_a_set_is_refused_on_route_requests(twins):
    re = twins.cached
    b = twins.batch(re)
    b.set_caches(twins.cached_caches, twins.idx)
    before = _launch(re, b)
    assert re.last_route() == capi.ROUTE_REQUESTS and re.last_launch()["family"] == capi.KERNEL_PACKED_REQUESTS
    plain = twins.batch(re)
    _launch(re, plain)
    assert re.last_route() == capi.ROUTE_PACKED
    assert "predict-only" in _refused(lambda: re.learn_batch(b, capi.MODE_HOGWILD, True))
    assert re.last_route() == capi.ROUTE_REQUESTS
    assert np.array_equal(_bits(_launch(re, b)), _bits(before)) and re.last_route() == capi.ROUTE_REQUESTS


def test_the_debug_kernel_version_survives_a_packed_launch(twins):
    f32, packed = twins.f32, twins.packed
    fb, pb = twins.batch(f32), twins.batch(packed)
    try:
        _launch(f32, fb)
        assert f32.last_launch()["family"] == capi.KERNEL_RESIDENT
        capi.check(f32.L.fwgpu_debug_set_kernel_version(f32.h, 1))
        _launch(f32, fb)
        assert f32.last_launch()["family"] == capi.KERNEL_VEC4
        # the packed gather exists in the resident kernel only: the launch plans for it whatever the setting says, and leaves the setting alone
        capi.check(packed.L.fwgpu_debug_set_kernel_version(packed.h, 1))
        p1 = _launch(packed, pb)
        assert packed.last_route() == capi.ROUTE_PACKED and packed.last_launch()["family"] == capi.KERNEL_PACKED
        p2 = _launch(packed, pb)
        assert packed.last_route() == capi.ROUTE_PACKED and packed.last_launch()["family"] == capi.KERNEL_PACKED
        assert np.array_equal(_bits(p1), _bits(p2))
        _launch(f32, fb)
        assert f32.last_launch()["family"] == capi.KERNEL_VEC4
    finally:
        capi.check(f32.L.fwgpu_debug_set_kernel_version(f32.h, 0))
        capi.check(packed.L.fwgpu_debug_set_kernel_version(packed.h, 0))
