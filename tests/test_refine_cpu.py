"""scal_refine_* without a GPU: the argument checks that precede the device, SCAL_E_NO_DEVICE where there is none, and the ctypes
mirrors of the two structs against the header's own layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(S, **kw):
    v = dict(max_corr_dist=2.0, transformation_epsilon=1e-6, fitness_epsilon=1e-6, fitness_gate=0.3, max_iterations=100, max_frames=4,
             max_points=1000, device=0)
    v.update(kw)
    return S.RefineConfig(**v)


def test_refine_argument_checks_and_no_device(S):
    L = S.lib()
    h = C.c_void_p()
    assert L.scal_refine_create(None, C.byref(h)) == S.E_ARG
    for bad in (dict(max_frames=0), dict(max_points=0), dict(max_points=-5), dict(max_iterations=0), dict(max_corr_dist=0.0),
                dict(max_corr_dist=float("nan")), dict(fitness_gate=float("nan"))):
        cfg = _cfg(S, **bad)
        assert L.scal_refine_create(C.byref(cfg), C.byref(h)) == S.E_ARG, bad
        assert b"scal_refine_create" in L.scal_last_error()
    cfg = _cfg(S)
    assert L.scal_refine_create(C.byref(cfg), None) == S.E_ARG
    rc = L.scal_refine_create(C.byref(cfg), C.byref(h))
    if S.device_count() < 1:
        assert rc == S.E_NO_DEVICE and not h.value
        with pytest.raises(S.ScalError) as e:
            S.MultiviewRefine(4, 1000)
        assert e.value.code == S.E_NO_DEVICE
    else:
        assert rc == S.OK and h.value
        L.scal_refine_destroy(h)
    off = np.array([0, 1], np.int32)
    P = np.zeros(12)
    res = (S.RefineFrameResult * 1)()
    run = C.c_int(0)
    for fn in (L.scal_refine_run, L.scal_refine_run_device):
        assert fn(None, None, off.ctypes.data_as(C.POINTER(C.c_int)), 1, P.ctypes.data_as(C.POINTER(C.c_double)), None, 2.0, 1, res,
                  C.byref(run)) == S.E_ARG
    L.scal_refine_destroy(None)


def test_refine_struct_layouts_match_the_header(S, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scaloam_hip.h"\n'
                   'int main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(scal_refine_config), offsetof(scal_refine_config, fitness_gate),\n'
                   '           offsetof(scal_refine_config, max_iterations), offsetof(scal_refine_config, device), sizeof(scal_refine_frame_result),\n'
                   '           offsetof(scal_refine_frame_result, accepted), offsetof(scal_refine_frame_result, fitness),\n'
                   '           offsetof(scal_refine_frame_result, T));\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, B = S.RefineConfig, S.RefineFrameResult
    assert got == [C.sizeof(A), A.fitness_gate.offset, A.max_iterations.offset, A.device.offset, C.sizeof(B), B.accepted.offset,
                   B.fitness.offset, B.T.offset]
