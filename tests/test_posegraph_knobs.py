"""CPU: the pose-graph solver reads no hidden strategy switch from the environment.  The SRRG2_AMD_PG_* variables
posegraph.hip hands to getenv are exactly those of the srrg2_posegraph_tuning fields, plus SRRG2_AMD_PG_OFFSET_LIMIT (the
test hook of the device structure build's fallback); a new one has to be declared here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "csrc", "posegraph.hip")

# srrg2_posegraph_tuning field -> the variable that overrides its default at create
TUNING_VARIABLES = {
    "match_passes": "SRRG2_AMD_PG_PASSES",
    "two_phase": "SRRG2_AMD_PG_TWO_PHASE",
    "use_graph": "SRRG2_AMD_PG_GRAPH",
    "debug": "SRRG2_AMD_PG_DEBUG",
    "keep_structure": "SRRG2_AMD_PG_KEEP_STRUCTURE",
    "omega_p": "SRRG2_AMD_PG_OMEGA_P",
    "omega": "SRRG2_AMD_PG_OMEGA",
    "lag_below": "SRRG2_AMD_PG_LAG",
    "device_structure": "SRRG2_AMD_PG_DEVICE_STRUCTURE",
}


def _source():
    txt = open(SRC).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//[^\n]*", "", txt)


def _variables_read():
    """names passed to getenv, directly or through the create-time helpers geti / getf (whose getenv takes `name`)"""
    txt = _source()
    args = re.findall(r"\bgetenv\s*\(\s*([^)]*?)\s*\)", txt)
    assert args, "no getenv call found in posegraph.hip"
    names = set()
    for a in args:
        m = re.fullmatch(r'"(\w+)"', a)
        if m:
            names.add(m.group(1))
        else:  # (a helper's parameter: what its callers pass)
            assert a == "name", "getenv with a computed argument: " + a
    names.update(re.findall(r'\bget[if]\s*\(\s*"(\w+)"', txt))
    return names


def test_the_tuning_table_covers_every_field():
    from srrg2_slam_interfaces_amd.posegraph import PoseGraphTuning

    fields = {f for f, _ in PoseGraphTuning._fields_} - {"reserved_"}
    assert fields == set(TUNING_VARIABLES)


def test_the_environment_holds_no_hidden_switch():
    read = _variables_read()
    assert all(n.startswith("SRRG2_AMD_PG_") for n in read), sorted(read)
    assert read == set(TUNING_VARIABLES.values()) | {"SRRG2_AMD_PG_OFFSET_LIMIT"}
