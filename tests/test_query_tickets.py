"""The host rules of the ticketed queries (edyn_amd/csrc/query_tickets.hpp: the table of outstanding tickets - limits, stale tickets,
collection in any order, release and refill - and the argument rules of the submits: ignore offsets, want masks, flags, the capacity
rule) - plain C++ without HIP, checked by tests/cpp/query_tickets.cpp against values written from the rules' statements. The program
has its own main and links no library; it is built a second time with the address and undefined-behaviour sanitizers where the
toolchain has their runtime, and runs as that stand-alone program. No GPU needed."""
import os
import subprocess

import pytest
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "query_tickets.cpp")


def _build(out, extra=()):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-o", out, SRC], capture_output=True, text=True, timeout=300)


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "QUERY_TICKETS_OK" in out.stdout, out.stdout + out.stderr


def test_query_tickets(tmp_path):
    exe = str(tmp_path / "query_tickets")
    b = _build(exe)
    assert b.returncode == 0, b.stderr
    _run(exe)


def test_query_tickets_sanitized(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    have = subprocess.run(["g++", *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True, timeout=300)
    if have.returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "query_tickets_san")
    b = _build(exe, san)
    assert b.returncode == 0, b.stderr
    _run(exe)
