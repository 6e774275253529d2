"""The drop-in filter's SetPointScalarImage() on the GPU (itk/tests/point_scalars_update.cxx): GetPointScalars() and the output
mesh's point data against a host loop over the mesh's points through itk::LinearInterpolateImageFunction plus the inside test,
exactly, on the static and the dynamic mesh traits; off again an empty accessor and no point data; the refusals with the host
walk and with several devices -- the program exits non-zero on a difference."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_drop_in_filter_point_scalars_update():
    exe = os.path.join(ROOT, "midas-journal-740_amd", "itk", "build", "point_scalars_update")
    if not os.path.exists(exe):
        pytest.fail("itk/build/point_scalars_update is missing: __graft_entry__.build() makes it")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout.strip(), run.stderr.strip())
    assert run.returncode == 0 and "identical" in run.stdout
    assert "host walk with a second image: refused" in run.stdout
    assert "two devices with a second image: refused" in run.stdout
    assert run.stdout.count("0 differ from the host loop, 0 point data differ") == 2
    assert run.stdout.count("off again: empty, no point data, the same mesh") == 2
