"""scal_pipeline's four busy lanes (stage_lane: 0, 1, 3, 4) each run on a hardware queue of their own.

Two streams on one queue run their packets in order, so lanes that share a queue stop overlapping and a scan costs the sum of their
chains.  Plain streams come from the runtime's queue pool (GPU_MAX_HW_QUEUES), which torch's null stream and any earlier stream already
use; the library's lanes must not depend on what is left of it.  scal_debug_lane_queue (a diagnostic outside the public header) reports
the queue behind a lane's stream, read by a kernel from its dispatch packet."""
import ctypes as C
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUSY_LANES = (0, 1, 3, 4)

# run in this process and, with GPU_MAX_HW_QUEUES=1, in a fresh one: prints one line "<null queue> <lane queue> ..."
_CHECK = r"""
import ctypes as C, sys
import torch
sys.path.insert(0, sys.argv[1])
import scaloam as S

x = torch.arange(1 << 16, dtype=torch.float32, device="cuda") * 2.0  # torch's null stream is in use before the pipeline exists
torch.cuda.synchronize()
p = S.Pipeline(S.HDL64, 5.0, max_points=20000, max_map_points=200000, sc_max_keyframes=64)
L = S.lib()
L.scal_debug_lane_queue.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
qs = []
for lane in [-1] + [int(a) for a in sys.argv[2:]]:
    q = C.c_ulonglong(0)
    rc = L.scal_debug_lane_queue(0, lane, C.byref(q))
    assert rc == 0, (lane, rc, L.scal_last_error())
    qs.append(q.value)
p.close()
print(" ".join(str(q) for q in qs))
"""


def _queues(out):
    qs = [int(v) for v in out.strip().splitlines()[-1].split()]
    return qs[0], qs[1:]


def _assert_own_queues(null_q, lane_qs):
    assert all(q != 0 for q in [null_q] + lane_qs)
    assert len(set(lane_qs)) == len(BUSY_LANES), f"busy lanes share hardware queues: {dict(zip(BUSY_LANES, map(hex, lane_qs)))}"
    assert null_q not in lane_qs, "a busy lane shares the null stream's hardware queue"


def test_busy_lanes_have_own_queues(S):
    import torch

    x = torch.ones(1 << 16, device="cuda") * 3.0
    torch.cuda.synchronize()
    p = S.Pipeline(S.HDL64, 5.0, max_points=20000, max_map_points=200000, sc_max_keyframes=64)
    try:
        L = S.lib()
        L.scal_debug_lane_queue.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
        qs = []
        for lane in (-1,) + BUSY_LANES:
            q = C.c_ulonglong(0)
            assert L.scal_debug_lane_queue(0, lane, C.byref(q)) == 0, L.scal_last_error()
            qs.append(q.value)
    finally:
        p.close()
    del x
    _assert_own_queues(qs[0], qs[1:])


def test_busy_lanes_have_own_queues_with_one_pooled_queue():
    """GPU_MAX_HW_QUEUES=1 folds every plain stream onto one queue; the busy lanes must still get four of their own."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1")
    r = subprocess.run([sys.executable, "-c", _CHECK, os.path.join(ROOT, "sc-a-loam_amd", "python")] + [str(l) for l in BUSY_LANES],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _assert_own_queues(*_queues(r.stdout))
