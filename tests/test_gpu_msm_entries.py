"""The MSM's entries stage by itself (csrc/msm_entries.hpp: digits, the two-level sort, the order by bucket size, the large-bucket plan): the
program tests/cpp/entriestest.hip calls its three functions on buffers of its own and compares dig, offs, idx, order, plan, tasks and large with a
host restatement, over the shapes that reach each path of the stage (see the table of cases in its main)."""
import subprocess

import pytest

from harness import program

pytestmark = pytest.mark.gpu
CASES = 10


def test_entries_stage_unit():
    out = subprocess.run([program("entriestest")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert out.returncode == 0 and out.stdout.count(": ok (") == CASES, out.stdout
