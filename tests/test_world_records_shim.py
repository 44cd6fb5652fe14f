"""Contact entities and step callbacks on a multi-device world through the C++ shim (include/edyn/edyn.hpp, init_config::devices):
tests/cpp/multi_contacts.cpp runs one registry program - materialize_contacts, contact_point_data, pre / post step callbacks, a kick from
a callback, registry.destroy - on one device and on two shards; the two registries agree at every one of 150 updates (state and
presentation bit for bit, the same manifold and point entities with the same point data, manifold_exists, callback counts), across a
re-partition. tests/cpp/host_records.cpp holds the host side of the same path - import_records and the contact table - without a GPU.
One program at a time (one device process besides pytest)."""
import os
import subprocess

import pytest
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
PROGS = ["multi_contacts", "multi_contacts_entt"]


@pytest.mark.parametrize("prog", PROGS)
def test_multi_contacts_compiles(prog):
    subprocess.check_call(["make", "-s", "-C", CPP, prog])
    assert os.path.exists(os.path.join(CPP, prog))


@pytest.mark.parametrize("prog", ["host_records", "host_records_entt"])
def test_record_import_and_contact_table_on_the_host(prog):
    subprocess.check_call(["make", "-s", "-C", CPP, prog])
    out = subprocess.run([os.path.join(CPP, prog)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HOST_RECORDS_OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("prog", PROGS)
def test_contact_entities_and_callbacks_on_two_shards(prog):
    subprocess.check_call(["make", "-s", "-C", CPP, prog])
    out = subprocess.run([os.path.join(CPP, prog)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "MULTI_CONTACTS_OK" in out.stdout, out.stdout + out.stderr
