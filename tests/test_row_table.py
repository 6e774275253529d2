"""The host-only table of the mesh's rows and the optional outputs (csrc/tests/row_table.hip): the list of device buffers,
the emit's and the keep's reservation sizes against the formulas written out per row, every refusal of an attribute per route
and slab in full, and the rows' way back to their places before a count.  No GPU."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "midas-journal-740_amd", "csrc")


def test_row_table():
    subprocess.check_call(["make", "-s", "-C", CSRC, "build/row_table"])      # (make knows whether it is stale)
    run = subprocess.run([os.path.join(CSRC, "build", "row_table")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "row_table ok" in run.stdout, run.stdout + run.stderr
