"""The host rules of edynhip_world_edit_bodies (edyn_amd/csrc/world_rules.hpp "body edits": which shards take an edit, boundary
crossing, the owner of a body made dynamic, when the approach check is due, the inertia the scene writes out; and validate_body_edit as
the world calls it) are plain C++ without HIP, checked by tests/cpp/world_body_edit_rules.cpp. The program has its own main and links
no library; it is built a second time with the address and undefined-behaviour sanitizers where the toolchain has their runtime, and
runs as that stand-alone program. No GPU needed."""
import os
import subprocess

import pytest
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "world_body_edit_rules.cpp")


def _build(out, extra=()):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-o", out, SRC], capture_output=True, text=True, timeout=300)


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "WORLD_BODY_EDIT_RULES_OK" in out.stdout, out.stdout + out.stderr


def test_world_body_edit_rules(tmp_path):
    exe = str(tmp_path / "world_body_edit_rules")
    b = _build(exe)
    assert b.returncode == 0, b.stderr
    _run(exe)


def test_world_body_edit_rules_sanitized(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    have = subprocess.run(["g++", *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True, timeout=300)
    if have.returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    exe = str(tmp_path / "world_body_edit_rules_san")
    b = _build(exe, san)
    assert b.returncode == 0, b.stderr
    _run(exe)
