"""ctypes binding of the reference's serving FFI as libfwgpu.so exports it (include/fw_ffi.h, lib.rs:150-236) --
the same calls a JNI / ctypes client of the reference's libfw makes."""
import ctypes as C

import numpy as np

from . import _capi as capi


def _lib():
    L = capi.lib()
    if not getattr(L, "_fw_ffi_ready", False):
        L.new_fw_predictor_prototype.argtypes = [C.c_char_p]
        L.new_fw_predictor_prototype.restype = C.c_void_p
        L.clone_lite.argtypes = [C.c_void_p]
        L.clone_lite.restype = C.c_void_p
        for name in ("fw_predict", "fw_predict_with_cache", "fw_setup_cache"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_char_p]
            getattr(L, name).restype = C.c_float
        L.free_predictor.argtypes = [C.c_void_p]
        L.free_predictor.restype = None
        L.fwgpu_predictor_predict_batch.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.c_void_p]
        L.fwgpu_predictor_predict_batch.restype = C.c_int
        L.fwgpu_predictor_predict_text.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.fwgpu_predictor_predict_text.restype = C.c_int
        L.fwgpu_predictor_last_text_route.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.fwgpu_predictor_last_text_route.restype = C.c_int
        L.fwgpu_predictor_predict_requests.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.c_uint32),
                                                       C.POINTER(C.c_void_p)]
        L.fwgpu_predictor_predict_requests.restype = C.c_int
        L.fwgpu_predictor_apply_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.fwgpu_predictor_apply_diff.restype = C.c_int
        L._fw_ffi_ready = True
    return L


def predict_requests(predictors, requests):
    """The candidates of several requests in ONE launch (fwgpu_predictor_predict_requests): predictors[r] -- the prototype and clone_lite copies of one
    model, each after its own setup_cache -- scores requests[r], a list of str or the array Predictor.encode_batch made of one.  Returns one float32
    array per request: what predict_with_cache returns per line, -1.0 for a line that does not parse."""
    if len(predictors) != len(requests):
        raise ValueError("one list of lines per predictor")
    L = _lib()
    n = len(predictors)
    arrs = [t if isinstance(t, C.Array) else Predictor.encode_batch(t) for t in requests]
    outs = [np.zeros(len(a), dtype=np.float32) for a in arrs]
    handles = (C.c_void_p * max(n, 1))(*[p.p for p in predictors])
    inputs = (C.POINTER(C.c_char_p) * max(n, 1))(*[C.cast(a, C.POINTER(C.c_char_p)) for a in arrs])
    counts = (C.c_uint32 * max(n, 1))(*[len(a) for a in arrs])
    out_ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data if o.size else None for o in outs])
    capi.check(L.fwgpu_predictor_predict_requests(handles, n, inputs, counts, out_ptrs))
    return outs


class Predictor:
    def __init__(self, command: str = None, _ptr=None):
        self.L = _lib()
        self.p = _ptr if _ptr is not None else self.L.new_fw_predictor_prototype(command.encode())
        if not self.p:
            raise capi.FwgpuError(-1, self.L.fwgpu_last_error().decode(errors="replace"))

    def clone_lite(self):
        return Predictor(_ptr=self.L.clone_lite(self.p))

    def predict(self, text: str) -> float:
        return float(self.L.fw_predict(self.p, text.encode()))

    def setup_cache(self, text: str) -> float:
        return float(self.L.fw_setup_cache(self.p, text.encode()))

    def predict_with_cache(self, text: str) -> float:
        return float(self.L.fw_predict_with_cache(self.p, text.encode()))

    @staticmethod
    def encode_batch(texts):
        """the char** a C / Rust caller already holds: build it once, outside any timed region"""
        return (C.c_char_p * len(texts))(*[t.encode() for t in texts])

    def predict_batch(self, texts, with_cache=False) -> np.ndarray:
        """texts: a list of str, or the array Predictor.encode_batch made of one"""
        arr = texts if isinstance(texts, C.Array) else self.encode_batch(texts)
        out = np.zeros(len(arr), dtype=np.float32)
        capi.check(self.L.fwgpu_predictor_predict_batch(self.p, arr, len(arr), int(with_cache), capi.ptr(out)))
        return out

    def predict_text(self, text: bytes, with_cache=False, cap=None) -> np.ndarray:
        """a request as one text, a candidate per line, scanned on the device: what predict_batch returns for the lines (each with its
        newline); with a device cache the lines never become records on the host (fwgpu_predictor_predict_text)"""
        cap = text.count(b"\n") + 1 if cap is None else cap
        out = np.zeros(max(cap, 1), dtype=np.float32)
        n = C.c_uint64()
        capi.check(self.L.fwgpu_predictor_predict_text(self.p, text, len(text), int(with_cache), capi.ptr(out), cap, C.byref(n)))
        return out[: n.value]

    def last_text_route(self):
        """(lines of the last predict_text, lines of those the host parsed, whether the call went through predict_batch)"""
        n, h, f = C.c_uint64(), C.c_uint64(), C.c_int()
        capi.check(self.L.fwgpu_predictor_last_text_route(self.p, C.byref(n), C.byref(h), C.byref(f)))
        return n.value, h.value, bool(f.value)

    def apply_diff(self, diff: bytes):
        """patches a --packed_weights model in place from the byte-diff stream of the file it was loaded from and the next published file
        (persistence.Image.diff / diff_bytes); the prototype and every clone_lite copy see it -- fwgpu_predictor_apply_diff"""
        d = np.frombuffer(diff, dtype=np.uint8)
        capi.check(self.L.fwgpu_predictor_apply_diff(self.p, capi.ptr(d), d.size))

    def close(self):
        if self.p:
            self.L.free_predictor(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
