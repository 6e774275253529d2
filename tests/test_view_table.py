"""The host-only table of the source views (csrc/tests/view_table.hip): resolve_view over every kind, route, projection
feature and pair, framed_desc against cuberille_region_desc and the padded description.  No GPU."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "midas-journal-740_amd", "csrc")


def test_view_table():
    subprocess.check_call(["make", "-s", "-C", CSRC, "build/view_table"])      # (make knows whether it is stale)
    run = subprocess.run([os.path.join(CSRC, "build", "view_table")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "view_table ok" in run.stdout, run.stdout + run.stderr
