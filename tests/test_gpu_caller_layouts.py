"""Every cloud entry point on the layouts callers hand in (tests/layout_cases.py): records of 12 .. 44 bytes with the normal
inside and junk behind it, host and device memory, K clouds pooled behind decoy records with offsets tables that do not start at 0.

The reference of every case is the same call on a fresh handle fed what the layout denotes -- packed arrays, offsets from 0,
normals in arrays of their own -- and "equal" means bit for bit: every byte of the srrg2_batch_result records, and what the handle
exposes afterwards (status, estimate, iteration statistics, correspondence count, H, the cue slices' records).  The packed single
compute() and compute_batch are held to the float64 oracle (helpers.assert_same_run).  After every call has returned, the
caller's buffers are overwritten with moved points before anything is read back: a call that returned before its ingest had
read them, or a getter that went back to them, shows.  tests/test_layout_cases.py proves on the oracle that a kernel which
ignored the base of an offsets table would give another answer on these cases."""
import ctypes as C

import numpy as np
import pytest

import consensus_cases as cc
import consensus_restatement as cr
import layout_cases as lc
from helpers import assert_same_run, cue_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5  # srrg2_error codes of the C ABI
HOST, DEVICE = abi.MEM_HOST, abi.MEM_DEVICE
MEMS = [pytest.param(HOST, id="host"), pytest.param(DEVICE, id="device")]
SE3, SE2 = lc.SE3, lc.SE2
I32 = C.POINTER(C.c_int32)


# ---- the caller's memory ---------------------------------------------------------------------------------------------------------
class Memory:
    """the caller's buffers of one test, in host or device memory (srrg2_amd_device_malloc / srrg2_amd_memcpy); overwrite()
    changes one in place, close() frees the device buffers"""

    def __init__(self, lib):
        lib.srrg2_amd_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        lib.srrg2_amd_device_malloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        lib.srrg2_amd_device_free.argtypes = [C.c_void_p]
        self.lib, self.bufs = lib, []

    def place(self, arr, mem):
        """a buffer of the caller's holding `arr`: dict(addr, mem, arr); the host copy is the caller's own"""
        arr = np.ascontiguousarray(arr).copy()
        b = dict(mem=mem, arr=arr, addr=arr.ctypes.data, dev=None)
        if mem != HOST:
            p = C.c_void_p()
            assert self.lib.srrg2_amd_device_malloc(C.c_size_t(arr.nbytes + 64), C.byref(p)) == 0
            b["dev"], b["addr"] = p, p.value
            self.overwrite(b, arr)
        self.bufs.append(b)
        return b

    def overwrite(self, b, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == b["arr"].nbytes
        if b["mem"] == HOST:
            b["arr"].view(np.uint8).reshape(-1)[:] = arr.view(np.uint8).reshape(-1)
        elif arr.nbytes:
            assert self.lib.srrg2_amd_memcpy(b["dev"], C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), 1, None) == 0

    def close(self):
        for b in self.bufs:
            if b["dev"] is not None:
                self.lib.srrg2_amd_device_free(b["dev"])
        self.bufs = []


@pytest.fixture
def memory(product):
    from srrg2_slam_interfaces_amd import _capi

    m = Memory(_capi.lib())
    yield m
    m.close()


class Placed:
    """a records layout in the caller's memory: the four cloud arguments of the C calls (coords, stride, normals, stride)"""

    def __init__(self, memory, layout, mem, gate, separate_normals=None):
        self.memory, self.layout, self.gate = memory, layout, gate
        self.b = memory.place(layout["buf"], mem)
        self.nb = None
        self.coords, self.cs, self.normals, self.ns = self.b["addr"], layout["stride"], 0, 0
        if separate_normals is not None:  # (records for the points, a packed array for the normals)
            self.nb = memory.place(lc.records(separate_normals, None, layout["dim"] * 4), mem)
            self.normals, self.ns = self.nb["addr"], layout["dim"] * 4
        elif layout["normal_at"] is not None:
            self.normals, self.ns = self.b["addr"] + layout["normal_at"], layout["stride"]
        elif layout["nbuf"] is not None:
            self.nb = memory.place(layout["nbuf"], mem)
            self.normals, self.ns = self.nb["addr"], layout["nstride"]

    def args(self):
        return (_vp(self.coords), C.c_int(self.cs), _vp(self.normals), C.c_int(self.ns))

    def scribble(self):
        """the call has returned: the caller reuses its buffers (every point moved by a third of the gate, normals turned)"""
        self.memory.overwrite(self.b, lc.moved(self.layout["buf"], self.layout["dim"], self.gate))
        if self.nb is not None:
            n = self.nb["arr"].view(np.float32)
            self.memory.overwrite(self.nb, np.ascontiguousarray(-n[:, ::-1]))


def _vp(addr):
    return C.c_void_p(addr) if addr else None


# ---- the calls, on raw pointers ----------------------------------------------------------------------------------------------------
def _results(K, fill=None):
    res = (abi.BatchResult * max(K, 1))()
    if fill is not None:
        C.memset(res, fill, C.sizeof(res))
    return res


def _guesses(al, guesses):
    return np.ascontiguousarray(np.asarray(guesses, np.float32).reshape(len(guesses), al.tsize))


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _set_cloud(al, which, si, placed, n, mem):
    al._check(al._b.fn(which)(al._h, C.c_int(si), *placed.args(), C.c_int(n), C.c_int(mem)))


def _compute_batch(al, placed, offsets, mem, guesses, res=None):
    K = len(offsets) - 1
    res = _results(K) if res is None else res
    g = _guesses(al, guesses)
    rc = al._b.fn("compute_batch")(al._h, C.c_int(K), *placed.args(), offsets.ctypes.data_as(I32), C.c_int(mem), _fptr(g), res)
    return rc, res


def _compute_batch_correspondences(al, placed, offsets, mem, recs, corr_offsets, guesses, res=None):
    K = len(offsets) - 1
    res = _results(K) if res is None else res
    g = _guesses(al, guesses)
    rc = al._b.fn("compute_batch_correspondences")(al._h, C.c_int(K), *placed.args(), offsets.ctypes.data_as(I32), C.c_int(mem),
                                                   C.c_void_p(recs.ctypes.data), corr_offsets.ctypes.data_as(I32), _fptr(g), res)
    return rc, res


def _align_pairs(al, fixed, foff, moving, moff, mem, guesses, res=None):
    K = len(foff) - 1
    res = _results(K) if res is None else res
    g = _guesses(al, guesses)
    rc = al._b.lib.srrg2_align_pairs(al._h, C.c_int(K), *fixed.args(), foff.ctypes.data_as(I32), *moving.args(), moff.ctypes.data_as(I32),
                                     C.c_int(mem), _fptr(g), res)
    return rc, res


def _align_batch_slices(al, entries, mem, guesses, res=None):
    """entries: {slice: (Placed, offsets)}; every other slice gets a null entry"""
    K = len(guesses)
    res = _results(K) if res is None else res
    arr = (abi.BatchSliceClouds * len(al.slices))()
    for si, (p, off) in entries.items():
        e = arr[si]
        e.coords, e.coord_stride_bytes = C.cast(C.c_void_p(p.coords), C.POINTER(C.c_float)), p.cs
        if p.normals:
            e.normals, e.normal_stride_bytes = C.cast(C.c_void_p(p.normals), C.POINTER(C.c_float)), p.ns
        e.offsets = off.ctypes.data_as(I32)
    g = _guesses(al, guesses)
    rc = al._b.lib.srrg2_align_batch_slices(al._h, C.c_int(K), C.c_int(len(al.slices)), arr, C.c_int(mem), _fptr(g), res)
    return rc, res


# ---- what is compared --------------------------------------------------------------------------------------------------------------
def _record_bytes(res, K):
    """the K result records, byte for byte (the library zeroes a record before it fills it)"""
    raw = bytes(res)
    size = C.sizeof(abi.BatchResult)
    return [raw[k * size:(k + 1) * size] for k in range(K)]


def _handle_state(al, cue=(0,), records=True):
    st = dict(status=al.status(), estimate=al.moving_in_fixed().tobytes(), stats=al.iteration_stats(),
              num_correspondences=al.num_correspondences(), information=al.information().tobytes())
    if records:
        for si in cue:
            st["corr%d" % si] = al.correspondences(si).tobytes()
            st["fstat%d" % si] = al.factor_status(si).tobytes()
    return st


def _assert_same_batch(got, want, K):
    a, b = _record_bytes(got, K), _record_bytes(want, K)
    for k in range(K):
        assert a[k] == b[k], "result record %d of %d differs from the packed run's" % (k, K)


def _assert_same_state(got, want):
    assert got.keys() == want.keys()
    for key in want:
        assert got[key] == want[key], key


# ---- 1. set_fixed / set_moving + compute() ---------------------------------------------------------------------------------------
def _single_handle(lib, c, oracle=False):
    al = lib.OracleAligner(c["kind"]) if oracle else lib.MultiAligner(c["kind"])
    al.set_params(max_iterations=lc.ITERATIONS)
    al.add_slice(c["cfg"])
    return al


_SINGLE = {}


def _single_reference(product, oracle, dim, with_normals):
    """the packed run of the single case (set_fixed / set_moving on packed arrays, normals in arrays of their own), held to the
    oracle once; computed once per (dim, normals) and shared"""
    key = (dim, with_normals)
    if key not in _SINGLE:
        c = lc.single_case(dim)
        d = c["data"]
        runs = []
        for lib, is_oracle in ((oracle, True), (product, False)):
            al = _single_handle(lib, c, is_oracle)
            al.set_fixed(0, d["fixed"], d["fixed_normals"] if with_normals else None)
            al.set_moving(0, d["moving"], d["moving_normals"] if with_normals else None)
            al.set_moving_in_fixed(syn.identity(dim))
            assert al.compute() == abi.SUCCESS
            runs.append(al)
        assert_same_run(*runs)
        if dim == 2:
            assert runs[1].last_compute_path() & abi.PATH_ONE_WORKGROUP
        _SINGLE[key] = (c, _handle_state(runs[1]))
    return _SINGLE[key]


def _run_single(product, memory, c, fixed, moving, mem, scribble=True, kept=False):
    """set_fixed / set_moving from two layouts (lc.single) in `mem`, the buffers overwritten once each call has returned"""
    d = c["data"]
    al = _single_handle(product, c)
    for which, layout, n in (("set_fixed", fixed, len(d["fixed"])), ("set_moving", moving, len(d["moving"]))):
        p = layout if isinstance(layout, Placed) else Placed(memory, layout, mem, c["gate"])
        _set_cloud(al, which, 0, p, n, mem)
        if scribble:
            p.scribble()
    al.set_moving_in_fixed(syn.identity(al.dim))
    assert al.compute() == abi.SUCCESS
    return _handle_state(al)


@pytest.mark.parametrize("dim,stride", [(d, s) for d in (3, 2) for s in lc.STRIDES[d]])
def test_compute_from_host_records_of_every_stride(product, oracle, memory, dim, stride):
    """the normal inside the record wherever it has room (a status word behind it); dim 3 at 12 and 16 bytes: records for the
    points, a packed array for the normals; dim 2 at 8 and 12 bytes: no normals.  The buffers are overwritten as soon as
    set_fixed / set_moving have returned"""
    with_normals = dim == 3 or lc.holds_normals(dim, stride)
    c, want = _single_reference(product, oracle, dim, with_normals)
    d = c["data"]
    fixed = lc.single(d["fixed"], d["fixed_normals"] if with_normals else None, stride)
    moving = lc.single(d["moving"], d["moving_normals"] if with_normals else None, stride)
    assert lc.unpack_records(fixed["buf"], dim)[0].tobytes() == d["fixed"].tobytes()
    _assert_same_state(_run_single(product, memory, c, fixed, moving, HOST), want)


@pytest.mark.parametrize("stride", [16, 32])
def test_compute_from_device_records(product, oracle, memory, stride):
    c, want = _single_reference(product, oracle, 3, True)
    d = c["data"]
    fixed, moving = lc.single(d["fixed"], d["fixed_normals"], stride), lc.single(d["moving"], d["moving_normals"], stride)
    _assert_same_state(_run_single(product, memory, c, fixed, moving, DEVICE), want)


@pytest.mark.parametrize("mem", MEMS)
def test_compute_with_normals_of_another_stride(product, oracle, memory, mem):
    """44-byte point records whose own normal slot is junk, the normals in a packed array"""
    c, want = _single_reference(product, oracle, 3, True)
    d = c["data"]
    fixed = Placed(memory, lc.single(d["fixed"], None, 44), mem, c["gate"], separate_normals=d["fixed_normals"])
    moving = Placed(memory, lc.single(d["moving"], None, 44), mem, c["gate"], separate_normals=d["moving_normals"])
    assert (fixed.cs, fixed.ns) == (44, 12)
    _assert_same_state(_run_single(product, memory, c, fixed, moving, mem), want)


@pytest.mark.parametrize("mem", MEMS)
def test_one_workgroup_sort_reads_the_callers_records(product, oracle, memory, mem):
    """SE(2), 380 points: the sort of set_moving reads the 20-byte records (staged, or in place in device memory) itself"""
    c, want = _single_reference(product, oracle, 2, True)
    d = c["data"]
    fixed, moving = lc.single(d["fixed"], d["fixed_normals"], 20), lc.single(d["moving"], d["moving_normals"], 20)
    _assert_same_state(_run_single(product, memory, c, fixed, moving, mem), want)


# ---- 2. compute_batch --------------------------------------------------------------------------------------------------------------
_BATCH = {}


def _batch_handle(lib, d, oracle=False):
    al = lib.OracleAligner(d["kind"]) if oracle else lib.MultiAligner(d["kind"])
    al.set_params(max_iterations=lc.ITERATIONS)
    al.add_slice(lc.cue3())
    al.set_fixed(0, d["fixed"], d["fixed_normals"])
    return al


def _batch_reference(product, oracle, K, with_normals):
    """the packed compute_batch of lc.batch_clouds(K), held to the oracle's loop (every record, and the handle's state of
    alignment K - 1 with assert_same_run); once per (K, normals)"""
    key = (K, with_normals)
    if key not in _BATCH:
        d = lc.batch_clouds(K, 3000 if K <= 4 else 1500)
        normals = d["moving_normals"] if with_normals else None
        al = _batch_handle(product, d)
        res = al.compute_batch(d["moving"], d["guesses"], normals)
        assert sum(r["status"] == abi.SUCCESS for r in res) == (K - 1 if K > 1 else 1)
        ref = _batch_handle(oracle, d, True)
        ores = ref.compute_batch(d["moving"], d["guesses"], normals)
        for k in range(K):
            assert ores[k]["moving_in_fixed"].tobytes() == res[k]["moving_in_fixed"].tobytes(), k
            assert (ores[k]["status"], ores[k]["num_iterations"], ores[k]["last"]) == (res[k]["status"], res[k]["num_iterations"], res[k]["last"]), k
        assert_same_run(ref, al)
        _BATCH[key] = (d, res._raw, _handle_state(al))
    return _BATCH[key]


def _check_compute_batch(product, oracle, memory, K, lead, stride, mem, with_normals):
    d, want, want_state = _batch_reference(product, oracle, K, with_normals)
    pool = lc.pooled(d["moving"], d["moving_normals"] if with_normals else None, lead, stride, lc.GATE3)
    placed = Placed(memory, pool, mem, lc.GATE3)
    al = _batch_handle(product, d)
    rc, res = _compute_batch(al, placed, pool["offsets"], mem, d["guesses"])
    assert rc == 0
    placed.scribble()  # (the call has returned: correspondences / factor_status of alignment K - 1 come from the handle)
    _assert_same_batch(res, want, K)
    _assert_same_state(_handle_state(al), want_state)
    return al


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("with_normals", [False, True], ids=["bare", "normals"])
@pytest.mark.parametrize("stride", [12, 28])
@pytest.mark.parametrize("lead", [1, 257])
def test_compute_batch_on_pooled_clouds(product, oracle, memory, lead, stride, with_normals, mem):
    """K = 4 (an empty cloud at k = 1), the clouds behind `lead` decoy records; 12 bytes with normals: an array of their own"""
    _check_compute_batch(product, oracle, memory, 4, lead, stride, mem, with_normals)


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("lead,stride,with_normals", [(257, 28, True), (1, 12, False)])
def test_compute_batch_of_one_and_of_pipelined_parts(product, oracle, memory, K, lead, stride, with_normals, mem):
    """K = 1 behind a lead (its problem table starts at 0); K = 20 of up to 1 500 points: the batch runs as parts on streams of
    their own, every part's sort from the pool's base"""
    al = _check_compute_batch(product, oracle, memory, K, lead, stride, mem, with_normals)
    if K == 20:  # (what plan_batch_parts asks of a batch before it splits it)
        t = al.tuning()
        d = _batch_reference(product, oracle, K, with_normals)[0]
        assert t.batch_pipeline != 0 and not t.fast_batch_queue and max(len(m) for m in d["moving"]) > t.small_max_points


# ---- 3. compute_batch_correspondences ----------------------------------------------------------------------------------------------
def _given_handle(product, d):
    c = abi.default_slice_config(SE3)
    c.kind, c.finder, c.robustifier, c.robustifier_chi_threshold = abi.SLICE_P2P, abi.FINDER_CORRESPONDENCES, abi.ROBUST_CAUCHY, 0.05
    al = product.MultiAligner(SE3)
    al.set_params(max_iterations=lc.ITERATIONS)
    al.add_slice(c)
    al.set_fixed(0, d["fixed"], None)
    return al


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("lead,clead", [(1, 1), (257, 5)])
def test_compute_batch_correspondences_on_pooled_clouds_and_records(product, memory, lead, clead, mem):
    d = lc.landmarks()
    K = len(d["moving"])
    sizes = [len(m) for m in d["moving"]]
    ref = _given_handle(product, d)
    want = ref.compute_batch_correspondences(d["moving"], d["corrs"], d["guesses"])
    assert sum(r["status"] == abi.SUCCESS for r in want) == K - 1
    want_state = _handle_state(ref)
    pool = lc.pooled(d["moving"], None, lead, 28, 0.3)
    pc = lc.pooled_corrs(d["corrs"], clead, len(d["fixed"]), min(n for n in sizes if n))
    placed = Placed(memory, pool, mem, 0.3)
    al = _given_handle(product, d)
    rc, res = _compute_batch_correspondences(al, placed, pool["offsets"], mem, pc["recs"], pc["offsets"], d["guesses"])
    assert rc == 0
    _assert_same_batch(res, want._raw, K)
    _assert_same_state(_handle_state(al), want_state)
    # one more record per alignment whose moving_idx lies beyond its own cloud but inside the pool: what the packed run does
    # with it (the library refuses the call, the results untouched), the pooled run does -- it is not read from the neighbour
    extra = []
    for k, c in enumerate(d["corrs"]):
        e = np.zeros(1 if sizes[k] else 0, lc.CORR)
        e["moving_idx"], e["response"] = sizes[k] + 1, 2.0
        extra.append(np.concatenate([c, e]))
    assert all(lead + sum(sizes[:k + 1]) + 1 < len(pool["buf"]) for k in range(K))
    pe = lc.pooled_corrs(extra, clead, len(d["fixed"]), min(n for n in sizes if n))
    packed = Placed(memory, lc.pooled(d["moving"], None, 0, 12, 0.3, tail=0), HOST, 0.3)
    packed_recs, packed_off = np.concatenate(extra), np.concatenate([[0], np.cumsum([len(e) for e in extra])]).astype(np.int32)
    rc_ref, res_ref = _compute_batch_correspondences(ref, packed, packed.layout["offsets"], HOST, packed_recs, packed_off, d["guesses"],
                                                     _results(K, 0xAB))
    rc, res = _compute_batch_correspondences(al, placed, pool["offsets"], mem, pe["recs"], pe["offsets"], d["guesses"], _results(K, 0xAB))
    assert rc == rc_ref == E_INVALID
    assert bytes(res) == bytes(res_ref) == b"\xab" * (K * C.sizeof(abi.BatchResult))
    # ... and the handle goes on: the same bits again
    rc, res = _compute_batch_correspondences(al, placed, pool["offsets"], mem, pc["recs"], pc["offsets"], d["guesses"])
    assert rc == 0
    _assert_same_batch(res, want._raw, K)


# ---- 4. srrg2_align_pairs ------------------------------------------------------------------------------------------------------------
def _pairs_case(name):
    if name == "se2":
        return dict(kind=SE2, cfg=lc.cue2(), gate=lc.GATE2, strides=(20, 12), pairs=lc.scans(4))
    cfg = lc.cue3() if name == "p2plane" else cue_config(SE3, abi.SLICE_P2P, lc.GATE3, abi.ROBUST_CAUCHY, 0.05, 0.8)
    return dict(kind=SE3, cfg=cfg, gate=lc.GATE3, strides=(28, 16), pairs=lc.pair_clouds())


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("name", ["p2plane", "p2p", "se2"])
def test_align_pairs_on_two_pools(product, memory, name, mem):
    """the fixed pool at 28 bytes behind 5 decoys (normals inside), the moving pool at 16 bytes behind 3 (normals in an array
    of their own); SE(2): 20 and 12 bytes, 400 points, the one-workgroup path"""
    c = _pairs_case(name)
    pairs, dim = c["pairs"], abi.point_dim(c["kind"])
    K = len(pairs)
    ident = [syn.identity(dim)] * K

    def handle():
        al = product.MultiAligner(c["kind"])
        al.set_params(max_iterations=lc.ITERATIONS)
        al.add_slice(c["cfg"])
        return al

    ref = handle()
    want = ref.compute_batch_pairs([p["fixed"] for p in pairs], [p["moving"] for p in pairs], ident,
                                   [p["fixed_normals"] for p in pairs], [p["moving_normals"] for p in pairs])
    assert sum(r["status"] == abi.SUCCESS for r in want) == K - 1
    want_state = _handle_state(ref, records=False)
    fpool = lc.pooled([p["fixed"] for p in pairs], [p["fixed_normals"] for p in pairs], lc.PAIR_LEADS[0], c["strides"][0], c["gate"])
    mpool = lc.pooled([p["moving"] for p in pairs], [p["moving_normals"] for p in pairs], lc.PAIR_LEADS[1], c["strides"][1], c["gate"])
    assert fpool["normal_at"] is not None and mpool["nbuf"] is not None
    f, m = Placed(memory, fpool, mem, c["gate"]), Placed(memory, mpool, mem, c["gate"])
    al = handle()
    rc, res = _align_pairs(al, f, fpool["offsets"], m, mpool["offsets"], mem, ident)
    assert rc == 0
    f.scribble()
    m.scribble()
    _assert_same_batch(res, want._raw, K)
    _assert_same_state(_handle_state(al, records=False), want_state)
    if name == "se2":
        assert al.last_compute_path() & abi.PATH_ONE_WORKGROUP
    # by contract a pair batch leaves no pair records
    for fn in (al.correspondences, al.factor_status):
        with pytest.raises(RuntimeError, match=r"code %d" % E_STATE):
            fn(0)


# ---- 5. srrg2_align_batch_slices -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("name", ["nn2", "c3"])
def test_align_batch_slices_on_pooled_entries(product, memory, name, mem):
    """nn2: two nearest-neighbour cue slices whose entries have leads and strides of their own (2 / 28 bytes with the normals
    inside, 259 / 16 bytes without normals) and a prior slice with a null entry; c3: the projective pack, the owning slice's
    entry pooled behind 259 decoys, the sharing slice's entry null"""
    case = lc.nn2_case() if name == "nn2" else lc.c3_case()
    K = len(case["guesses"])
    ref = product.MultiAligner(case["kind"])
    case["setup"](ref)
    want = ref.compute_batch_slices(case["moving"], case["guesses"], case["moving_normals"])
    assert sum(r["status"] == abi.SUCCESS for r in want) >= K - 1
    want_state = _handle_state(ref, case["cue"])
    entries, placed = {}, []
    for si, (lead, stride) in lc.SLICE_LAYOUT[name].items():
        pool = lc.pooled(case["moving"][si], case["moving_normals"][si], lead, stride, case["gates"][si])
        p = Placed(memory, pool, mem, case["gates"][si])
        entries[si] = (p, pool["offsets"])
        placed.append(p)
    al = product.MultiAligner(case["kind"])
    case["setup"](al)
    rc, res = _align_batch_slices(al, entries, mem, case["guesses"])
    assert rc == 0
    for p in placed:
        p.scribble()
    _assert_same_batch(res, want._raw, K)
    _assert_same_state(_handle_state(al, case["cue"]), want_state)


# ---- 6. srrg2_consensus_compute --------------------------------------------------------------------------------------------------------
CONSENSUS_FIELDS = ("status", "best_hypothesis", "num_inliers", "num_pairs", "num_valid_pairs", "num_degenerate", "num_rejected",
                    "num_scored", "cost_exponent", "cost")


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("dim", [2, 3])
def test_consensus_on_pooled_clouds_and_records(product, memory, dim, mem):
    """moving_offsets[0] = 6 and corr_offsets[0] = 4, 16-byte records: the restatement on what the layout denotes, bit for bit"""
    c = cc.batch5(dim, seed=14)
    tau = c["params"].get("inlier_distance", cr.DEFAULTS["inlier_distance"])
    pool = lc.pooled(c["movings"], None, 6, 16, 3 * tau)
    pc = lc.pooled_corrs(c["corrs"], 4, len(c["fixed"]), len(c["movings"][0]))
    want = cr.consensus(dim, c["fixed"], lc.unpack(pool)[0], lc.unpack(pc), **c["params"])
    v = product.ConsensusVerifier(dim)
    try:
        fixed = memory.place(lc.records(c["fixed"], None, 16), mem)
        moving = Placed(memory, pool, mem, 3 * tau)
        raw = v.compute_raw(fixed["addr"], 16, len(c["fixed"]), moving.coords, 16, pool["offsets"], mem, pc["recs"], pc["offsets"],
                            v.params(**c["params"]), capacity=len(pc["recs"]))
        got = v._unpack(raw[0], raw[1], raw[2])
    finally:
        v.close()
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for f in CONSENSUS_FIELDS:
            assert g[f] == w[f], (k, f, g[f], w[f])
        assert g["moving_in_fixed"].tobytes() == w["moving_in_fixed"].tobytes(), k
        assert g["inliers"].tobytes() == w["inliers"].tobytes(), k


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def _untouched(res, K):
    return bytes(res) == b"\xab" * (max(K, 1) * C.sizeof(abi.BatchResult))


def _neg(offsets):
    out = offsets.copy()
    out[0] = -1
    return out


def test_a_negative_first_offset_is_refused_by_compute_batch(product, oracle, memory):
    d, want, _ = _batch_reference(product, oracle, 4, True)
    pool = lc.pooled(d["moving"], d["moving_normals"], 5, 28, lc.GATE3)
    placed = Placed(memory, pool, HOST, lc.GATE3)
    al = _batch_handle(product, d)
    assert _compute_batch(al, placed, pool["offsets"], HOST, d["guesses"])[0] == 0
    rc, res = _compute_batch(al, placed, _neg(pool["offsets"]), HOST, d["guesses"], _results(4, 0xAB))
    assert rc == E_INVALID and _untouched(res, 4)
    rc, res = _compute_batch(al, placed, pool["offsets"], HOST, d["guesses"])
    assert rc == 0
    _assert_same_batch(res, want, 4)


def test_a_negative_first_offset_is_refused_by_compute_batch_correspondences(product, memory):
    """both tables.  The records are a view a few records inside a larger allocation: a build that copied from in front of
    corr_offsets[0] = -1 would still read inside it"""
    d = lc.landmarks()
    K = len(d["moving"])
    pool = lc.pooled(d["moving"], None, 5, 28, 0.3)
    pc = lc.pooled_corrs(d["corrs"], 3, len(d["fixed"]), 100)
    room = np.concatenate([np.zeros(8, lc.CORR), pc["recs"]])
    recs = room[8:]
    assert recs.base is room and recs.ctypes.data == room.ctypes.data + 8 * lc.CORR.itemsize
    placed = Placed(memory, pool, HOST, 0.3)
    al = _given_handle(product, d)
    rc, good = _compute_batch_correspondences(al, placed, pool["offsets"], HOST, recs, pc["offsets"], d["guesses"])
    assert rc == 0
    for off, coff in ((pool["offsets"], _neg(pc["offsets"])), (_neg(pool["offsets"]), pc["offsets"])):
        rc, res = _compute_batch_correspondences(al, placed, off, HOST, recs, coff, d["guesses"], _results(K, 0xAB))
        assert rc == E_INVALID and _untouched(res, K), (off[0], coff[0])
    rc, res = _compute_batch_correspondences(al, placed, pool["offsets"], HOST, recs, pc["offsets"], d["guesses"])
    assert rc == 0
    _assert_same_batch(res, good, K)


def test_a_negative_first_offset_is_refused_by_align_pairs(product, memory):
    c = _pairs_case("p2plane")
    pairs = c["pairs"]
    K = len(pairs)
    ident = [syn.identity(3)] * K
    fpool = lc.pooled([p["fixed"] for p in pairs], [p["fixed_normals"] for p in pairs], 5, 28, c["gate"])
    mpool = lc.pooled([p["moving"] for p in pairs], None, 3, 16, c["gate"])
    f, m = Placed(memory, fpool, HOST, c["gate"]), Placed(memory, mpool, HOST, c["gate"])
    al = product.MultiAligner(SE3)
    al.set_params(max_iterations=lc.ITERATIONS)
    al.add_slice(c["cfg"])
    rc, good = _align_pairs(al, f, fpool["offsets"], m, mpool["offsets"], HOST, ident)
    assert rc == 0
    for foff, moff in ((_neg(fpool["offsets"]), mpool["offsets"]), (fpool["offsets"], _neg(mpool["offsets"]))):
        rc, res = _align_pairs(al, f, foff, m, moff, HOST, ident, _results(K, 0xAB))
        assert rc == E_INVALID and _untouched(res, K), (foff[0], moff[0])
    rc, res = _align_pairs(al, f, fpool["offsets"], m, mpool["offsets"], HOST, ident)
    assert rc == 0
    _assert_same_batch(res, good, K)


def test_a_negative_first_offset_is_refused_by_align_batch_slices(product, memory):
    case = lc.nn2_case()
    K = len(case["guesses"])
    entries = {}
    for si, (lead, stride) in lc.SLICE_LAYOUT["nn2"].items():
        pool = lc.pooled(case["moving"][si], case["moving_normals"][si], lead, stride, case["gates"][si])
        entries[si] = (Placed(memory, pool, HOST, case["gates"][si]), pool["offsets"])
    al = product.MultiAligner(case["kind"])
    case["setup"](al)
    rc, good = _align_batch_slices(al, entries, HOST, case["guesses"])
    assert rc == 0
    for si in entries:
        bad = dict(entries)
        bad[si] = (entries[si][0], _neg(entries[si][1]))
        rc, res = _align_batch_slices(al, bad, HOST, case["guesses"], _results(K, 0xAB))
        assert rc == E_INVALID and _untouched(res, K), si
    rc, res = _align_batch_slices(al, entries, HOST, case["guesses"])
    assert rc == 0
    _assert_same_batch(res, good, K)


def test_a_negative_first_offset_is_refused_by_consensus_compute(product):
    c = cc.batch5(3, seed=14)
    K = len(c["movings"])
    pool = lc.pooled(c["movings"], None, 6, 16, 0.15)
    pc = lc.pooled_corrs(c["corrs"], 4, len(c["fixed"]), len(c["movings"][0]))
    fixed = np.ascontiguousarray(c["fixed"], np.float32)
    v = product.ConsensusVerifier(3)
    params = v.params(**c["params"])

    def call(moff, coff):
        res = np.full(K * C.sizeof(abi.ConsensusResult), 0xAB, np.uint8)
        inl = np.full(len(pc["recs"]) * lc.CORR.itemsize, 0xAB, np.uint8)
        offs = np.full(K + 1, -77, np.int64)
        rc = v._lib.srrg2_consensus_compute(v._h, fixed.ctypes.data, C.c_int(12), C.c_int(len(fixed)), C.c_int(K), pool["buf"].ctypes.data,
                                            C.c_int(16), moff.ctypes.data_as(I32), C.c_int(HOST), pc["recs"].ctypes.data,
                                            coff.ctypes.data_as(I32), C.byref(params), res.ctypes.data, inl.ctypes.data,
                                            C.c_int64(len(pc["recs"])), offs.ctypes.data_as(C.POINTER(C.c_int64)))
        return rc, res.tobytes() + inl.tobytes() + offs.tobytes(), bool((res == 0xAB).all() and (inl == 0xAB).all() and (offs == -77).all())

    try:
        rc, good, _ = call(pool["offsets"], pc["offsets"])
        assert rc == 0
        for moff, coff in ((_neg(pool["offsets"]), pc["offsets"]), (pool["offsets"], _neg(pc["offsets"]))):
            rc, _, untouched = call(moff, coff)
            assert rc == E_INVALID and untouched, (moff[0], coff[0])
        rc, again, _ = call(pool["offsets"], pc["offsets"])
        assert rc == 0 and again == good
    finally:
        v.close()
