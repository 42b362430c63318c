"""The MSM's entries stage by itself (csrc/msm_entries.hpp: digits, the two-level sort, the order by bucket size, the large-bucket plan): the
program tests/cpp/entriestest.hip calls its three functions on buffers of its own and compares dig, offs, idx, order, plan, tasks and large with a
host restatement, over the shapes that reach each path of the stage (see the table of cases in its main)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = 10


def test_entries_stage_unit():
    exe = os.path.join(ROOT, "tests", "cpp", "entriestest")
    assert os.path.exists(exe), "tests/cpp/entriestest is missing: python -c 'import __graft_entry__ as g; g.build()'"
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert out.returncode == 0 and out.stdout.count(": ok (") == CASES, out.stdout
