"""The development knobs (EDYNHIP_* environment variables) are read in one function of the library, from one table; the list in
scripts/README.md and the variables the tests set are checked against that table. Source checks only: no GPU, no library."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edyn_amd", "csrc")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _sources():
    return {f: _read(os.path.join(CSRC, f)) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp"))}


def _table_names():
    src = _read(os.path.join(CSRC, "capi.hip"))
    table = src[src.index("kKnobTable[] = {"):]
    table = table[:table.index("\n};")]
    names = re.findall(r'^\s*\{"(EDYNHIP_[A-Z0-9_]+)", KNOB_(?:ON|OFF|SET|NUM|PATH), -?\d+, ', table, re.M)
    assert len(names) == len(table.strip().split("\n")) - 1, "a row of kKnobTable does not look like the others"
    assert len(names) == len(set(names)) and len(names) > 20
    return set(names)


def test_the_environment_is_read_in_one_function():
    src = _sources()
    calls = [(f, m.start()) for f, s in src.items() for m in re.finditer(r"\bgetenv\s*\(", s)]
    assert [f for f, _ in calls] == ["capi.hip"], calls   # one call in the whole library ...
    capi = src["capi.hip"]
    body = capi[capi.index("Knobs read_knobs() {"):]
    body = body[:body.index("\n}\n")]
    assert body.count("getenv(") == 1 and "getenv(r.name)" in body   # ... inside read_knobs, over the table's names
    for f, s in src.items():   # and no EDYNHIP_ name is handed to anything that could read it elsewhere
        assert not re.search(r'getenv\s*\(\s*"', s), f
        assert not re.search(r"\b(secure_getenv|environ)\b", s), f


def test_the_readme_lists_the_same_knobs_as_the_table():
    readme = _read(os.path.join(ROOT, "scripts", "README.md"))
    section = readme[readme.index("Environment knobs read by the library"):]
    listed = re.findall(r"^\| `(EDYNHIP_[A-Z0-9_]+)` \|", section, re.M)
    assert len(listed) == len(set(listed))
    assert set(listed) == _table_names()


def test_every_knob_a_test_sets_is_in_the_table():
    table = _table_names()
    constants = set(re.findall(r"\bEDYNHIP_[A-Z0-9_]+", _read(os.path.join(ROOT, "include", "edynhip.h"))))
    set_by_tests = set()
    for d, _, files in os.walk(os.path.join(ROOT, "tests")):
        for f in files:
            if not f.endswith((".py", ".cpp", ".hpp", ".sh")) or f == os.path.basename(__file__):
                continue
            s = _read(os.path.join(d, f))
            # os.environ["X"] = / environ.get / pop / setdefault, monkeypatch.setenv / delenv, env dictionaries of subprocesses, setenv() in C++
            set_by_tests |= set(re.findall(r'(?:environ(?:\.\w+\(|\[)|setenv\(|delenv\(|putenv\(|env\[|dict\(os\.environ, )\s*[\'"]?(EDYNHIP_[A-Z0-9_]+)', s))
            set_by_tests |= set(re.findall(r'[\'"](EDYNHIP_[A-Z0-9_]+)[\'"]\s*:', s))   # a key of an environment dictionary
            set_by_tests |= set(re.findall(r"\b(EDYNHIP_[A-Z0-9_]+)=", s))              # NAME=value: a keyword of dict(os.environ, ...), a command line, a docstring
    set_by_tests -= {"EDYNHIP_LIB"}   # which library the Python package loads: not read by the library
    assert set_by_tests, "the pattern found no knob at all"
    assert {"EDYNHIP_NP_FUSED", "EDYNHIP_QUERY_SCAN_RATIO", "EDYNHIP_DATAFLOW"} <= set_by_tests
    assert not (set_by_tests - constants - table), sorted(set_by_tests - constants - table)


# ---- completeness of tests/test_knob_paths.py: a new knob or a new path without a parity test fails here
# Knobs that the matrix of test_knob_paths.py does not run. Only two kinds may stand here: knobs that print or write developer output and
# change nothing the step computes, and knobs whose parity test lives in another file (named beside each).
EXEMPT_OUTPUT_ONLY = {
    "EDYNHIP_DF_TRACE", "EDYNHIP_DFP_TRACE", "EDYNHIP_DF_TRACE_STEP",   # timestamps of one dataflow solve, written to a file
    "EDYNHIP_BP_STATS", "EDYNHIP_TREE_STATS",                           # figures on stderr
    "EDYNHIP_PP_PROF",                                                  # phase profile on stderr
    "EDYNHIP_WORLD_TRACE",                                              # wall times of a re-partition on stderr
}
EXEMPT_TESTED_ELSEWHERE = {
    "EDYNHIP_COL_LDS": "tests/test_gpu_parity.py::test_colouring_rounds_in_lds_and_in_global_memory_colour_alike",
    "EDYNHIP_NP_FUSED": "tests/test_np_fused.py",
    "EDYNHIP_QUERY_SCAN_RATIO": "tests/test_query_aabb.py",
}


def _matrix_module():
    import sys
    tests = os.path.join(ROOT, "tests")
    for p in (ROOT, tests):
        if p not in sys.path:
            sys.path.insert(0, p)
    import test_knob_paths
    return test_knob_paths


def test_every_knob_has_a_row_in_the_path_matrix_or_a_stated_exemption():
    table = _table_names()
    in_matrix = _matrix_module().knobs_in_matrix()
    assert in_matrix <= table, sorted(in_matrix - table)
    exempt = EXEMPT_OUTPUT_ONLY | set(EXEMPT_TESTED_ELSEWHERE)
    assert not (exempt & in_matrix), sorted(exempt & in_matrix)
    assert exempt <= table, sorted(exempt - table)   # (a knob that left the table leaves this list too)
    assert table - in_matrix - exempt == set(), sorted(table - in_matrix - exempt)
    for k in EXEMPT_OUTPUT_ONLY:
        assert re.search(r"_TRACE|_STATS$|^EDYNHIP_PP_PROF$", k), k
    for k, where in EXEMPT_TESTED_ELSEWHERE.items():   # the named test exists and sets the knob
        path = where.split("::")[0]
        src = _read(os.path.join(ROOT, path))
        assert k in src, (k, where)
        if "::" in where:
            assert "def %s(" % where.split("::")[1] in src, where


def test_every_path_bit_of_the_header_is_required_by_a_row_of_the_matrix():
    header = _read(os.path.join(ROOT, "include", "edynhip.h"))
    bits = re.findall(r"^#define EDYNHIP_PATH_([A-Z0-9_]+)\s+\(1ull << (\d+)\)", header, re.M)
    assert len(bits) >= 30 and len({b for _, b in bits}) == len(bits) == len({n for n, _ in bits})
    from edyn_amd import _capi
    assert _capi.PATH_BITS == {n: 1 << int(b) for n, b in bits}   # the Python mirror of the header
    required = _matrix_module().bits_required_by_matrix()
    assert required <= {n for n, _ in bits}, sorted(required - {n for n, _ in bits})
    assert {n for n, _ in bits} - required == set(), sorted({n for n, _ in bits} - required)


def test_every_row_of_the_matrix_names_a_scene_and_shows_a_path():
    m = _matrix_module()
    ids = [m._row_id(r) for r in m.MATRIX]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    assert set(m.INERT_ROWS) <= set(ids), sorted(set(m.INERT_ROWS) - set(ids))   # (a row that left the table leaves this list too)
    for knobs, scene, steps, need, clear in m.MATRIX:   # a row that must select nothing names no bit of its own
        if m._row_id((knobs, scene, steps, need, clear)) in m.INERT_ROWS:
            assert all(b.startswith("=") for b in need) and clear
    for knobs, scene, steps, need, clear in m.MATRIX:
        assert scene in m.SCENES and isinstance(steps, int)
        assert not ({b.lstrip("=") for b in need} & clear)
        if knobs and not (need or clear):
            raise AssertionError("a row that asserts no path bit proves nothing: %s" % m._row_id((knobs, scene, steps, need, clear)))
