"""CPU: the aligner reads no hidden strategy switch.  The variables aligner_host.hip, kernels.hip and kernels_prep.hip hand to
getenv are exactly those of the srrg2_aligner_tuning fields, plus SRRG2_AMD_TIMELINE / SRRG2_AMD_HOSTTIME (instrumentation) and
SRRG2_AMD_FUSED_GRID_MAX (the test hook of the fused grid kernel); the only strategy_mask bits the sources test are the two
named in include/srrg2_slam_amd.h; and no kernel source reads a strategy word.  A new one has to be declared here."""
import os
import re

from srrg2_slam_interfaces_amd import _abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "csrc")
HOST = ("aligner_host.hip", "kernels.hip", "kernels_prep.hip")
DEVICE = ("kernels.hip", "kernels_prep.hip", "kernels.h", "device_types.h", "device_util.h", "det_math.h")
HEADER = os.path.join(ROOT, "include", "srrg2_slam_amd.h")

# srrg2_aligner_tuning field -> the variable that overrides its default at create
TUNING_VARIABLES = {
    "strategy_mask": "SRRG2_AMD_TUNE",
    "queue_probe_iteration": "SRRG2_AMD_QPROBE",
    "small_max_points": "SRRG2_AMD_SMALL_MAX",
    "fast_from_iteration": "SRRG2_AMD_FAST_FROM",
    "fast_points_per_thread": "SRRG2_AMD_FAST_PPT",
    "fast_min_points": "SRRG2_AMD_FAST_MIN",
    "fast_gather": "SRRG2_AMD_FAST_GATHER",
    "fast_batch_queue": "SRRG2_AMD_FAST_QUEUE",
    "queue_min_points": "SRRG2_AMD_QUEUE_MIN",
    "msort_segments": "SRRG2_AMD_MSORT_SEGMENTS",
    "msort_key_bits": "SRRG2_AMD_MSORT_BITS",
    "lds_tile": "SRRG2_AMD_LDS_TILE",
    "cell_target": "SRRG2_AMD_CELL_TARGET",
    "rmax_cap": "SRRG2_AMD_RMAX_CAP",
    "search_lists": "SRRG2_AMD_SEARCH_LISTS",
    "search_team": "SRRG2_AMD_SEARCH_TEAM",
    "batch_pipeline": "SRRG2_AMD_BATCH_PIPELINE",
    "fused_control": "SRRG2_AMD_FUSED_CONTROL",
}
OTHER_VARIABLES = {"SRRG2_AMD_TIMELINE", "SRRG2_AMD_HOSTTIME", "SRRG2_AMD_FUSED_GRID_MAX"}
NAMED_BITS = {"SRRG2_TUNE_PROJ_SEPARATE_LAUNCHES": abi.TUNE_PROJ_SEPARATE_LAUNCHES, "SRRG2_TUNE_INIT_LAUNCH": abi.TUNE_INIT_LAUNCH}


def _source(path):
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//[^\n]*", "", txt)


def _variables_read():
    """names passed to getenv, directly or through the create-time helpers geti / getf (whose getenv takes `name`)"""
    names = set()
    for f in HOST:
        txt = _source(os.path.join(CSRC, f))
        for a in re.findall(r"\bgetenv\s*\(\s*([^)]*?)\s*\)", txt):
            m = re.fullmatch(r'"(\w+)"', a)
            if m:
                names.add(m.group(1))
            else:  # (a helper's parameter: what its callers pass)
                assert a == "name", "%s: getenv with a computed argument: %s" % (f, a)
        names.update(re.findall(r'\bget[if]\s*\(\s*"(\w+)"', txt))
    return names


def test_the_tuning_table_covers_every_field():
    fields = {f for f, _ in abi.AlignerTuning._fields_} - {"reserved_"}
    assert fields == set(TUNING_VARIABLES)


def test_the_environment_holds_no_hidden_switch():
    assert _variables_read() == set(TUNING_VARIABLES.values()) | OTHER_VARIABLES


def test_the_named_bits_are_the_only_ones_tested():
    hdr = _source(HEADER)
    defines = dict(re.findall(r"#define\s+(SRRG2_TUNE_\w+)\s+(.+)", hdr))
    for name, value in NAMED_BITS.items():
        m = re.fullmatch(r"\(1 << (\d+)\)", defines.pop(name).strip())
        assert m and 1 << int(m.group(1)) == value, name
    assert set(re.findall(r"\w+", defines.pop("SRRG2_TUNE_KNOWN_BITS"))) == set(NAMED_BITS)
    assert not defines, defines
    tested = set()
    for f in HOST:
        txt = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', _source(os.path.join(CSRC, f)))  # (messages name the field too)
        uses = re.findall(r"strategy_mask\b[^;,)]*", txt)
        for u in uses:
            if re.fullmatch(r"strategy_mask\s*=\s*0", u):  # (the default)
                continue
            if u.strip() == "strategy_mask":  # (geti's target)
                continue
            m = re.fullmatch(r"strategy_mask\s*&=?\s*~?\s*(\w+)", u.strip())
            assert m, "%s: strategy_mask used as `%s`" % (f, u)
            tested.add(m.group(1))
    assert tested == set(NAMED_BITS) | {"SRRG2_TUNE_KNOWN_BITS"}, tested


def test_no_kernel_source_reads_a_strategy_word():
    for f in DEVICE:
        txt = _source(os.path.join(CSRC, f))
        assert not re.search(r"\btune\b|strategy_mask|SRRG2_TUNE_", txt), f
