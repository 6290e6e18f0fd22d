"""Host-only pieces of the fp32 device operator: the new entries are exported
and declared, and the refusals that need no GPU (argument checks of
arpack_hip_csr_create_f32, CSR.from_arrays' dtype rules) answer before any HIP
call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["arpack_hip_csr_create_f32", "arpack_hip_csr_precision", "arpack_hip_csr_spmv_f32",
       "arpack_hip_csr_time_f32", "arpack_hip_csr_download_f32", "arpack_hip_ssaupd_csr",
       "arpack_hip_ssaupd_csr_cycles", "arpack_hip_snaupd_csr_cycles"]


def test_entries_exported_and_declared(pkg):
    hdr = open(os.path.join(ROOT, "include", "arpack_hip.h")).read()
    for name in NEW:
        assert hasattr(pkg.lib(), name), name
        assert re.search(r"\b%s\(" % name, hdr), name


def test_create_f32_bad_arguments(pkg):
    L = pkg.lib()
    h = C.c_void_p()
    rp = np.array([0, 1, 2], np.int64)
    col = np.array([0, 1], np.int32)
    val = np.array([1.0, 2.0], np.float32)
    args = (rp.ctypes.data, col.ctypes.data, val.ctypes.data)
    assert L.arpack_hip_csr_create_f32(None, 2, 2, *args) == -1
    assert L.arpack_hip_csr_create_f32(C.byref(h), 0, 0, *args) == -1
    assert L.arpack_hip_csr_create_f32(C.byref(h), 2, -1, *args) == -1
    assert L.arpack_hip_csr_create_f32(C.byref(h), 2, 2, None, col.ctypes.data, val.ctypes.data) == -1
    assert L.arpack_hip_csr_create_f32(C.byref(h), 2, 2, rp.ctypes.data, None, val.ctypes.data) == -1
    assert L.arpack_hip_csr_create_f32(C.byref(h), 2, 2, rp.ctypes.data, col.ctypes.data, None) == -1
    assert h.value is None
    assert L.arpack_hip_csr_precision(None) == -1
    assert L.arpack_hip_csr_spmv_f32(None, None, None) == -1
    assert L.arpack_hip_csr_time_f32(None, None, None, 1) == -1.0
    assert L.arpack_hip_csr_download_f32(None, None, None, None) == -1


def test_from_arrays_dtype_rules(pkg):
    rp = np.array([0, 1, 2], np.int64)
    col = np.array([0, 1], np.int32)
    val = np.array([1.0, 2.0])
    with pytest.raises(ValueError):  # an fp32 operator is square
        pkg.CSR.from_arrays(rp, col, val, shape=(2, 2), dtype=np.float32)
    with pytest.raises(ValueError):
        pkg.CSR.from_arrays(rp, col, val, dtype=np.float16)
