"""Run by tests/test_gpu_staged_winners.py::test_counters_of_the_stall_build in a process whose product library is the
-DSRRG2_FUSED_STALL build (SRRG2_AMD_LIB).  That build counts what became of the points decided from their staged sets
(srrg2_amd_debug_staged_winners, csrc/kernels.hip): every scenario must give the oracle's bits, and the counters must show that
twins are decided by their owner alone, that a neighbour which changes is fetched, and that a pass which still moves stages its
near-ties under the rule without the motion term -- and decides some."""
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
import staged_winner_scenarios as sw  # noqa: E402
from oracle import pyoracle as oracle  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi  # noqa: E402
from srrg2_slam_interfaces_amd import _capi  # noqa: E402

lib = _capi.lib()
assert "stall" in _capi.LIB_PATH, _capi.LIB_PATH
STAGED = ("staged", "decided", "rejected_overflow", "rejected_not_covered", "unstaged_failures", "too_many_thin")
WINNERS = ("kept", "changed_served", "changed_fetched", "near_tie_only", "owner_alone")


def counters():
    v, w = (C.c_ulonglong * 6)(), (C.c_ulonglong * 5)()
    assert lib.srrg2_amd_debug_staged_neighbours(v, 1) == 0
    assert lib.srrg2_amd_debug_staged_winners(w, 1) == 0
    return dict(zip(STAGED + WINNERS, [int(x) for x in v] + [int(x) for x in w]))


K3, PLANE = abi.SE3_QUAT_RIGHT, abi.SLICE_P2PLANE
counters()
out = {}
twins, near_ties = sc.with_twins(sc.pair(3))
assert near_ties >= 32, near_ties
sc.run_all(oracle, product, K3, PLANE, twins, [sc.FUSED])
out["twins"] = counters()
triplets, near_ties = sw.with_triplets(sc.pair(3))
assert near_ties >= 32, near_ties
sc.run_all(oracle, product, K3, PLANE, triplets, [sc.FUSED])
out["triplets"] = counters()
sc.run_all(oracle, product, K3, PLANE, twins, [dict(sc.FUSED, fast_from_iteration=1)])
out["motion"] = counters()
for k, v in out.items():
    print("staged winners,", k, v)
for v in out.values():
    assert v["kept"] + v["changed_fetched"] == v["decided"] and v["changed_served"] == 0, out
assert out["twins"]["owner_alone"] > 0 and out["twins"]["kept"] > 0, out
assert out["triplets"]["changed_fetched"] > 0, out
assert out["motion"]["near_tie_only"] > 0 and out["motion"]["decided"] > 0, out
print("WINNERS-OK")
