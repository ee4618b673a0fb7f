"""include/m6a.h's rule for data pointers -- all host or all device -- held entry point by entry point (the table and what is checked
for each row: tests/pointer_convention.py).  Every sentence asserted here is the library's own, in full."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import pointer_convention as PC                                                  # noqa: E402
from test_gpu_comm_stub import stub_lib                                          # noqa: E402,F401  (the fixture that builds tests/stub_rccl)


@pytest.fixture(scope="module")
def env():
    e = PC.Env()
    PC.prepare(e)
    yield e
    e.close()


@pytest.mark.parametrize("row", PC.TABLE, ids=[r.name for r in PC.TABLE])
def test_host_and_device_agree_and_every_refusal_is_clean(env, row):
    PC.check_row(env, row)


def test_gather_rows_on_the_stand_in_transport(stub_lib):
    """m6a_gather and m6a_gather_reads, one rank that is its own destination, in a process that binds the stand-in for librccl."""
    r = subprocess.run([sys.executable, os.path.join(PC.REPO, "tests", "pointer_convention.py"), "gather"], capture_output=True, text=True,
                       env=dict(os.environ, M6A_RCCL_LIB=stub_lib, HSA_ENABLE_IPC_MODE_LEGACY="0"), timeout=300)
    assert r.returncode == 0 and "gather rows ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
