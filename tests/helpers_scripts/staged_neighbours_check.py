"""Run by tests/test_gpu_staged_neighbours.py::test_counters_of_the_stall_build in a process whose product library is the
-DSRRG2_FUSED_STALL build (SRRG2_AMD_LIB).  That build counts what became of the staged neighbours of the converged passes
(srrg2_amd_debug_staged_neighbours, csrc/kernels.hip): every scenario must give the oracle's bits, and the counters must show
that the staged sets decided the ties, that a ball of 80 candidates was refused, and that a pass which still moves refuses."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch  # noqa: F401  (before the product library: tests/conftest.py)
except Exception:
    pass

import srrg2_slam_interfaces_amd as product  # noqa: E402
import staged_neighbour_scenarios as sc  # noqa: E402
from oracle import pyoracle as oracle  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi  # noqa: E402
from srrg2_slam_interfaces_amd import _capi  # noqa: E402

lib = _capi.lib()
assert "stall" in _capi.LIB_PATH, _capi.LIB_PATH
NAMES = ("staged", "decided", "rejected_overflow", "rejected_not_covered", "unstaged_failures", "too_many_thin")


def counters(reset=True):
    v = (C.c_ulonglong * 6)()
    assert lib.srrg2_amd_debug_staged_neighbours(v, 1 if reset else 0) == 0
    return dict(zip(NAMES, [int(x) for x in v]))


K3, PLANE = abi.SE3_QUAT_RIGHT, abi.SLICE_P2PLANE
counters()
out = {}
twins, near_ties = sc.with_twins(sc.pair(3))
assert near_ties >= 32, near_ties
sc.run_all(oracle, product, K3, PLANE, twins, [sc.FUSED])
out["ties"] = counters()
sc.run_all(oracle, product, K3, PLANE, sc.cropped(), [dict(sc.FUSED, fast_from_iteration=1)])
out["motion"] = counters()
sc.run_all(oracle, product, K3, PLANE, sc.with_clumps(sc.pair(3)), [sc.FUSED])
out["overflow"] = counters()
for k, v in out.items():
    print("staged neighbours,", k, v)
assert out["ties"]["staged"] > 0 and out["ties"]["decided"] > 0, out
assert out["motion"]["rejected_not_covered"] + out["motion"]["too_many_thin"] > 0, out
assert out["overflow"]["rejected_overflow"] > 0, out
print("STAGED-OK")
