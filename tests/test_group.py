"""The context group (include/cuberille_hip.h: cuberille_group_*) without a GPU: its cuts, its refusals, its exports and
the driver that times it.  tests/test_gpu_group.py runs it on the device."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GROUP_SYMBOLS = ["cuberille_group_create", "cuberille_group_destroy", "cuberille_group_last_error", "cuberille_group_context",
                 "cuberille_group_plan", "cuberille_group_warm_up", "cuberille_group_extract_host",
                 "cuberille_group_slab_result", "cuberille_group_mesh_host", "cuberille_group_release_host_mesh",
                 "cuberille_group_mesh_write_vtk", "cuberille_group_debug_fail_alloc"]


def _restated_plan(pkg, desc, params, n):
    """distributed.slab_range for min(n, Nz) slabs, each buffer widened by cuberille_required_halo and clipped."""
    below, above = pkg.required_halo(desc, params)
    nz = int(desc.dims[2])
    used = min(n, nz)
    out = []
    for r in range(used):
        z0, z1 = importlib.import_module(pkg.__name__ + ".distributed").slab_range(nz, used, r)
        out.append((z0, z1, max(z0 - below, 0), min(z1 + above, nz)))
    return out


def _tilted():
    a = np.deg2rad(20.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    return rz @ rx


CASES = [
    # dims, spacing, direction, max_steps, step
    ((64, 64, 64), (1.0, 1.0, 1.0), None, 50, -1.0),
    ((31, 17, 200), (1.0, 1.0, 0.25), None, 50, -1.0),
    ((40, 40, 97), (3.0, 1.7, 0.25), "tilted", 50, -1.0),
    ((20, 30, 55), (0.5, 0.5, 2.0), None, 5, 0.3),
    ((8, 8, 1000), (1.0, 1.0, 1.0), None, 400, 0.5),
    ((16, 16, 9), (1.0, 1.0, 1.0), "tilted", 0, -1.0),
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("n", [1, 2, 3, 8, 64])
def test_group_plan_equals_the_restated_cuts(pkg, case, n):
    dims, spacing, direction, max_steps, step = CASES[case]
    desc = pkg.make_desc(np.float32, dims, spacing, (0.5, -2.0, 7.0), _tilted() if direction else None)
    for project in (True, False):
        prm = pkg.make_params(0.0, project=project, max_steps=max_steps, step=step)
        assert pkg.group_plan(desc, prm, n) == _restated_plan(pkg, desc, prm, n)


def test_group_plan_uses_at_most_one_slab_per_slice(pkg):
    desc = pkg.make_desc(np.uint8, (10, 10, 5))
    prm = pkg.make_params(100)
    cuts = pkg.group_plan(desc, prm, 8)
    assert len(cuts) == 5
    assert [c[:2] for c in cuts] == [(z, z + 1) for z in range(5)]
    assert all(c[2] == 0 and c[3] == 5 for c in cuts)       # the halo reaches across the whole volume
    # the raw call: *n_used = min(n, Nz), bounds of the used slabs only
    bounds = (C.c_int64 * 32)(*([-7] * 32))
    used = C.c_int(-1)
    assert pkg._abi.lib().cuberille_group_plan(C.byref(desc), C.byref(prm), 8, bounds, C.byref(used)) == pkg._abi.OK
    assert used.value == 5 and list(bounds[20:32]) == [-7] * 12


def test_group_plan_refusals(pkg):
    desc = pkg.make_desc(np.float32, (32, 32, 32))
    prm = pkg.make_params(0.0)
    lib = pkg._abi.lib()
    used = C.c_int()
    bounds = (C.c_int64 * (4 * 65))()
    for n in (0, -1, 65):
        assert lib.cuberille_group_plan(C.byref(desc), C.byref(prm), n, bounds, C.byref(used)) == pkg._abi.ERR_ARGUMENT
    assert lib.cuberille_group_plan(C.byref(desc), C.byref(prm), 64, bounds, C.byref(used)) == pkg._abi.OK
    rg = pkg.make_params(0.0, gradient=pkg.cuberille.GRADIENT_RECURSIVE_GAUSSIAN)
    assert lib.cuberille_group_plan(C.byref(desc), C.byref(rg), 2, bounds, C.byref(used)) == pkg._abi.ERR_ARGUMENT
    with pytest.raises(pkg._abi.CuberilleError):
        pkg.group_plan(desc, rg, 2)
    # without projection the gradient is never evaluated: a slab takes it
    rg_flat = pkg.make_params(0.0, project=False, gradient=pkg.cuberille.GRADIENT_RECURSIVE_GAUSSIAN)
    assert len(pkg.group_plan(desc, rg_flat, 2)) == 2


def test_group_symbols_are_exported(pkg):
    pkg._abi.build()
    assert set(GROUP_SYMBOLS) <= set(pkg._abi.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in GROUP_SYMBOLS:
        assert name in defined, name
        assert getattr(pkg._abi.lib(), name) is not None


def test_group_create_refuses_sizes_and_names_the_member_without_a_device(pkg):
    lib = pkg._abi.lib()
    g = C.c_void_p()
    ids = (C.c_int * 65)()
    for n in (0, 65):
        assert lib.cuberille_group_create(C.byref(g), ids, n) == pkg._abi.ERR_ARGUMENT
        assert not g
    if lib.cuberille_device_count() > 0:
        return
    with pytest.raises(pkg._abi.CuberilleError) as e:
        pkg.ExtractorGroup([0, 0])
    assert e.value.code == pkg._abi.ERR_NO_DEVICE and "member 0" in str(e.value) and "no CPU fallback" in str(e.value)


def test_multi_update_driver_compiles_against_itk_lite(pkg):
    pkg._abi.build()
    itk = os.path.join(ROOT, "midas-journal-740_amd", "itk")
    subprocess.check_call(["make", "-s", "-C", itk, "build/multi_update"])
    exe = os.path.join(itk, "build", "multi_update")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run([exe, "16", "0,x"], capture_output=True, text=True)
    assert r.returncode == 2
    if pkg._abi.lib().cuberille_device_count() == 0:
        r = subprocess.run([exe, "16", "0,0"], capture_output=True, text=True)
        assert r.returncode == 1 and "cuberille_group_create" in r.stderr and "no CPU fallback" in r.stderr


def test_filter_devices_without_a_gpu(pkg):
    f = pkg.CuberilleImageToMeshFilter(device=0, devices=[0, 0])
    assert f.GetDevices() == [0, 0]
    f.SetDevices([])
    assert f.GetDevices() == []
    assert f.GetLastNumberOfSlabs() == 0
