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
