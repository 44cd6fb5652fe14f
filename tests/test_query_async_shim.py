"""edyn::raycast_async / query_aabb_async / query_aabb_of_interest_async through the C++ shim in execution_mode::asynchronous
(include/edyn/collision/raycast.hpp:170-182, query_aabb.hpp:37-44): tests/cpp/query_async.cpp on both registry branches - the same
scene and times in sequential mode (the synchronous queries give the expected answers after every update) and in asynchronous mode
(every delegate once, in id order, during the next update, bit for bit, with the registry holding the state of that answer); requests
before the first update, inside a delegate, on a destroyed entity and pending at detach; query_islands and the sequential modes'
refusals; and, built with EDYN_QUERY_IDS_CAPACITY = 4 (query_async_small.cpp), the capacity overflow. One program at a time."""
import os
import subprocess

import pytest
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
PROGS = ["query_async", "query_async_entt", "query_async_small", "query_async_small_entt"]


def test_shim_query_async_compiles_on_both_registry_branches():
    subprocess.check_call(["make", "-s", "-C", CPP] + PROGS)
    assert all(os.path.exists(os.path.join(CPP, p)) for p in PROGS)


@pytest.mark.gpu
@pytest.mark.parametrize("prog", PROGS)
def test_shim_query_async(prog):
    subprocess.check_call(["make", "-s", "-C", CPP, prog])
    out = subprocess.run([os.path.join(CPP, prog)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "QUERY_ASYNC_OK 1" in out.stdout, out.stdout + out.stderr
