"""Surface components on the GPU (cuberille_set_components): the library's three rows against the numpy reference of
tests/components_ref.py -- held to a breadth-first walk by tests/test_components.py -- on the library's own downloaded cells,
compared as bytes.  Every case also holds points, cells and counters to the bytes of the same extraction with the setting off.
The contended cases (comb, serpentine, isolated voxels) are ordinary inputs with defined answers.
"""
import os
import subprocess

import numpy as np
import pytest

import components_ref as ref
import test_components as cases
from conftest import ROOT, point_bytes
from test_cell_pixels import label_volume

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 4
KW = dict(threshold=0.5, step=-1.0, relax=0.95, max_steps=50)
COUNTERS = ("n_points", "n_cells", "verts_per_cell", "proj_iterations", "proj_stop_threshold", "proj_stop_steps", "n_escaped")


@pytest.fixture()
def ex(pkg):
    e = pkg.Extractor(0)
    yield e
    e.close()


def counters(res):
    return {k: int(getattr(res, k)) for k in COUNTERS}


def device_copy(vox):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(vox).view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return t


def same(got, want, what):
    cases.same(got, want, what)


def held(ex, mesh, what, offset=0):
    """The library's rows of the last extraction against the reference on the mesh's own cells -> the rows."""
    n = len(mesh.points)
    got = ex.download_components()
    want = ref.components(mesh.cells, n, offset)
    same(got, want, what)
    assert ex.n_components() == len(want[2]), what
    cases.check_properties(np.asarray(mesh.cells).astype(np.int64) - offset, n, got, what)
    ptrs = ex.components_device()
    assert [bool(p) for p in ptrs] == [n > 0, len(mesh.cells) > 0, len(want[2]) > 0], (what, ptrs)
    return got


def off_then_on(ex, run, what="", offset=0):
    """run() once with the setting off and once with it on: the mesh and the counters must be the same bytes, the rows the
    reference's.  Returns the mesh and the rows of the second run."""
    ex.set_components(False)
    r0 = run()
    m0, c0 = ex.download(), counters(r0)
    ex.set_components(True)
    r1 = run()
    m1 = ex.download()
    assert point_bytes(m0.points) == point_bytes(m1.points), (what, "the setting moved a point")
    assert m0.cells.tobytes() == m1.cells.tobytes(), (what, "the setting moved a cell")
    assert c0 == counters(r1), (what, c0, counters(r1))
    return m1, held(ex, m1, what, offset)


def params(pkg, iso=1, **kw):
    return pkg.make_params(iso, **dict(KW, **kw))


def test_one_voxel_pairs_and_the_empty_mesh(pkg, ex):
    for triangles in (0, 1):
        prm = params(pkg, project=0, triangles=triangles)
        mesh, (pc, cc, counts) = off_then_on(ex, lambda: ex.extract_host(pkg.Volume(cases.one_voxel()), prm), "one voxel")
        assert len(mesh.points) == 8 and len(mesh.cells) == 6 * (2 if triangles else 1) and len(counts) == 1
        assert not pc.any() and not cc.any() and int(counts[0]) == len(mesh.cells)
        for name, vox, k in (("corner", cases.pair(1, 1, 1), 1), ("edge", cases.pair(0, 1, 1), 1), ("separated", cases.pair(0, 0, 2), 2)):
            mesh, rows = off_then_on(ex, lambda: ex.extract_host(pkg.Volume(vox), prm), name)
            assert len(rows[2]) == k, (name, len(rows[2]))                      # (the lattice corner is one vertex)
            assert len(mesh.cells) == 12 * (2 if triangles else 1)
    # an empty mesh, all outside and all inside: K = 0, null device pointers, empty downloads -- on a context whose rows an
    # earlier mesh sized, and on a fresh one
    prm = params(pkg, project=1, triangles=1)
    fresh = pkg.Extractor(0)
    try:
        for e in (ex, fresh):
            for value in (0, 1):
                flat = pkg.Volume(np.full((9, 10, 11), value, dtype=np.uint8))
                mesh, (pc, cc, counts) = off_then_on(e, lambda: e.extract_host(flat, prm), "empty")
                assert len(mesh.cells) == 0 and pc.shape == cc.shape == counts.shape == (0,) and e.n_components() == 0
                assert e.components_device() == (None, None, None)
    finally:
        fresh.close()


@pytest.mark.parametrize("shift", (0, 1))
def test_isolated_voxels(pkg, ex, shift):
    """16 384 cubes that touch nothing.  With quirk Q1 off they are components of 8 points and 6 quads each, about 131 072 points
    (the mesh is the library's, the same bytes with the setting off: its sizes are not this test's to pin): 512 block sums, two
    blocks of their scan, the roots at a regular stride.  With the quirk on (the default) the cubes of a z column share vertices
    across the empty slices between them: no special case, the definition only reads the cells."""
    vox = cases.isolated_voxels(shift)
    vol, dev = pkg.Volume(vox), device_copy(vox)
    desc = pkg.make_desc(vox.dtype, vol.dims)
    prm = params(pkg, project=0, triangles=0, q1=False)
    for name, run in (("extract_host", lambda: ex.extract_host(vol, prm)), ("extract_device", lambda: ex.extract_device(dev.data_ptr(), desc, prm)),
                      ("extract_device, blind", lambda: ex.extract_device(dev.data_ptr(), desc, prm))):
        mesh, (pc, cc, counts) = off_then_on(ex, run, (name, shift))
        print(name, "points", len(mesh.points), "components", len(counts))
        # (what the case is for: the block sums of the scan and their scan both take more than one block)
        assert len(mesh.points) > 256 * 256 and len(counts) > 8192 and int(np.median(counts)) == 6
    mesh, rows = off_then_on(ex, lambda: ex.extract_host(vol, params(pkg, project=0, triangles=1)), ("quirk Q1", shift))
    assert 1 < len(rows[2]) < 16384


def test_comb_and_serpentine(pkg, ex):
    for name, vox in (("comb", cases.comb()), ("serpentine", cases.serpentine())):
        vol, dev = pkg.Volume(vox), device_copy(vox)
        desc = pkg.make_desc(vox.dtype, vol.dims)
        for triangles in (0, 1):
            prm = params(pkg, project=0, triangles=triangles)
            for route, run in (("extract_host", lambda: ex.extract_host(vol, prm)),
                               ("extract_device", lambda: ex.extract_device(dev.data_ptr(), desc, prm))):
                mesh, (pc, cc, counts) = off_then_on(ex, run, (name, triangles, route))
                assert len(counts) == 1 and int(counts[0]) == len(mesh.cells) and not pc.any() and not cc.any(), (name, len(counts))
                assert len(mesh.cells) > 4096


def test_noise_quads_and_triangles(pkg, ex):
    vox = cases.gradient_noise()
    vol = pkg.Volume(vox)
    ks = []
    for iso in cases.noise_isos(vox):
        mesh, quads = off_then_on(ex, lambda: ex.extract_host(vol, params(pkg, iso, project=1, triangles=0)), ("noise quads", iso))
        mesh, tris = off_then_on(ex, lambda: ex.extract_host(vol, params(pkg, iso, project=1, triangles=1)), ("noise triangles", iso))
        assert tris[0].tobytes() == quads[0].tobytes() and (tris[2] == 2 * quads[2]).all()
        assert np.array_equal(tris[1][0::2], quads[1]) and np.array_equal(tris[1][1::2], quads[1])
        ks.append(len(quads[2]))
    print("noise components:", ks)
    assert max(ks) >= 3


def test_views_with_normals_and_cell_pixels(pkg, ex):
    kw = dict(project=1, triangles=1)
    # a border on a volume whose object touches the edge: the surface closes there
    labels = label_volume((9, 11, 37), 8)
    assert labels[:, :, 0].any() and labels[0].any()
    ex.set_border(1, 0)
    off_then_on(ex, lambda: ex.extract_host(pkg.Volume(labels), params(pkg, 2, **kw)), "border")
    ex.set_border(0, 0)
    # a region that cuts an object in two pieces inside the box
    vox, start, size = cases.two_pieces_in_a_box()
    mesh, whole = off_then_on(ex, lambda: ex.extract_host(pkg.Volume(vox), params(pkg, 1, **kw)), "the whole U")
    assert len(whole[2]) == 1
    ex.set_region(start, size)
    dev = device_copy(vox)
    desc = pkg.make_desc(vox.dtype, pkg.Volume(vox).dims)
    for route, run in (("extract_host", lambda: ex.extract_host(pkg.Volume(vox), params(pkg, 1, **kw))),
                       ("extract_device", lambda: ex.extract_device(dev.data_ptr(), desc, params(pkg, 1, **kw)))):
        mesh, rows = off_then_on(ex, run, ("region", route))
        assert len(rows[2]) == 2, (route, len(rows[2]))
    ex.clear_region()
    # the band [1, 255] of a label volume, cell pixels and normals on as well: the pass reads the mesh, not the voxels
    ex.set_band(1, 255, 1, 0)
    ex.set_cell_pixels(True)
    ex.set_point_normals(True)
    mesh, rows = off_then_on(ex, lambda: ex.extract_host(pkg.Volume(labels), params(pkg, 1, **kw)), "band")
    assert len(rows[2]) >= 2
    pix, nrm = ex.download_cell_pixels(), ex.download_normals()
    assert pix.shape == (len(mesh.cells),) and (pix >= 1).all() and nrm.shape == (len(mesh.points), 3)
    ex.set_cell_pixels(False)
    ex.set_point_normals(False)
    ex.clear_band()


def test_three_meshes_on_one_context_and_memory(pkg):
    """Large, small, then a large one with more components than the small one has points: the rows blind-sized from history, too
    large, and grown; the setting toggled off in between; cuberille_debug_device_bytes returns to the figure of a context that
    never had it on."""
    large = cases.gradient_noise((24, 30, 70), seed=3)
    iso = cases.noise_isos(large)[1]
    small = cases.pair(0, 0, 2)
    many = cases.isolated_voxels()[:16, :40, :]
    seq = ((large, iso, True), (large, iso, True), (small, 1, True), (small, 1, True), (many, 1, False), (many, 1, False), (small, 1, True))
    got = {}
    for name in ("never", "used"):
        e = pkg.Extractor(0)
        try:
            devs = {}
            for i, (vox, v, q1) in enumerate(seq):
                dev = devs.setdefault(id(vox), device_copy(vox))
                desc = pkg.make_desc(vox.dtype, pkg.Volume(vox).dims)
                prm = params(pkg, v, project=1, triangles=1, q1=q1)
                if name == "used":
                    e.set_components(i != 3)                                    # (off for the second small one, then on again)
                e.extract_device(dev.data_ptr(), desc, prm)
                if name == "used" and i != 3:
                    rows = held(e, e.download(), ("sequence", i))
                    if vox is many:
                        assert len(rows[2]) == 8 * 20 * 32                      # more components than `small` has points (16)
            if name == "used":
                e.set_components(False)
            got[name] = e.device_bytes()
            if name == "used":
                e.extract_device(dev.data_ptr(), desc, prm)
                assert e.device_bytes() == got[name]
        finally:
            e.close()
    print("device bytes:", got)
    assert got["used"] == got["never"]


def test_count_emit_with_an_offset(pkg, ex):
    vox = cases.gradient_noise((20, 22, 70), seed=9)
    iso = cases.noise_isos(vox)[1]
    dev = device_copy(vox)
    desc = pkg.make_desc(vox.dtype, pkg.Volume(vox).dims)
    prm = params(pkg, iso, project=1, triangles=1)

    def count_emit(offset, ahead):
        ex.count(dev.data_ptr(), desc, prm)
        if ahead:
            ex.emit_points()
        return ex.emit(offset)

    mesh, base = off_then_on(ex, lambda: count_emit(0, False), "offset 0")
    for offset, ahead in ((1000, False), (77, True)):
        mesh, rows = off_then_on(ex, lambda: count_emit(offset, ahead), ("offset", offset), offset)
        assert int(mesh.cells.min()) >= offset
        same(rows, base, ("the labels never carry the offset", offset))
    def stream():
        return ex.extract_stream(desc, lambda dst, z0, z1: dst.__setitem__(slice(None), vox[z0:z1]), prm)
    mesh, rows = off_then_on(ex, stream, "extract_stream")
    same(rows, base, "extract_stream")


def test_state_capacity_and_refusals(pkg, ex):
    vox = cases.gradient_noise((20, 22, 70), seed=9)
    iso = cases.noise_isos(vox)[1]
    vol, dev = pkg.Volume(vox), device_copy(vox)
    desc = pkg.make_desc(vox.dtype, vol.dims)
    prm = params(pkg, iso, project=1, triangles=1)
    lib = pkg._abi.lib()

    def refused(fn):
        with pytest.raises(pkg._abi.CuberilleError) as e:
            fn()
        assert e.value.code == ARG and "components" in str(e.value), str(e.value)

    def plain():
        ex.extract_host(vol, prm)
        mesh = ex.download()
        held(ex, mesh, "plain")
        return mesh

    # the setting off: the getters answer ERR_STATE, before any mesh and after one
    for _ in range(2):
        for fn in (ex.download_components, ex.components_device, ex.n_components):
            with pytest.raises(pkg._abi.CuberilleError) as e:
                fn()
            assert e.value.code == STATE
        ex.extract_host(vol, prm)
    assert "components" in str(e.value)
    ex.set_components(True)
    with pytest.raises(pkg._abi.CuberilleError) as e:                           # (set, but the last extraction ran without)
        ex.download_components()
    assert e.value.code == STATE
    first = plain()
    # capacity_components below K
    k = ex.n_components()
    assert k >= 2
    counts = np.empty(k, dtype=np.uint64)
    assert lib.cuberille_components_download(ex._ctx, None, None, counts.ctypes.data, k - 1) == ARG
    assert lib.cuberille_components_download(ex._ctx, None, None, counts.ctypes.data, k) == 0
    assert int(counts.sum()) == len(first.cells)
    # a slab that is not the whole volume, the step calls: refused, and the context goes on
    slab = pkg._abi.Slab(global_nz=40, z_begin=10, own_z0=12, own_z1=16)
    refused(lambda: ex.extract_device(dev.data_ptr(), desc, prm, slab))
    refused(lambda: ex.count(dev.data_ptr(), desc, prm, slab))
    plain()
    refused(lambda: ex.step_begin(dev.data_ptr(), desc, prm))
    refused(lambda: ex.step_classify(dev.data_ptr(), desc, prm))
    plain()
    # a group with a member that has the setting on
    g = pkg.ExtractorGroup([0, 0])
    try:
        g.set_components(True)
        with pytest.raises(pkg._abi.CuberilleError) as e:
            g.extract_host(vol, prm)
        assert e.value.code == ARG and "components" in str(e.value)
        g.set_components(False)
        g.extract_host(vol, prm)
        assert point_bytes(g.download().points) == point_bytes(first.points)
    finally:
        g.close()
    # off after use: the last mesh stays, its components go; the next plain extraction is what it always was
    ex.set_components(False)
    with pytest.raises(pkg._abi.CuberilleError) as e:
        ex.download_components()
    assert e.value.code == STATE and "components" in str(e.value)
    assert point_bytes(ex.download().points) == point_bytes(first.points)
    ex.extract_host(vol, prm)
    assert ex.download().cells.tobytes() == first.cells.tobytes()


def parse_scalars(tok, at, n):
    assert tok[at:at + 6] == ["SCALARS", "component", "unsigned_int", "1", "LOOKUP_TABLE", "default"], tok[at:at + 6]
    return np.array([int(t) for t in tok[at + 6:at + 6 + n]], dtype=np.uint32), at + 6 + n


def test_vtk_blocks(pkg, ex, tmp_path):
    vox = label_volume((5, 6, 70), 3)
    vol = pkg.Volume(vox)
    prm = params(pkg, 1, project=1, triangles=1)
    never = pkg.Extractor(0)
    try:
        never.extract_host(vol, prm)
        plain = str(tmp_path / "never.vtk")
        never.write_vtk(plain)
    finally:
        never.close()
    base = open(plain, "rb").read()
    ex.set_components(True)
    ex.extract_host(vol, prm)
    pc, cc, counts = ex.download_components()
    assert len(counts) >= 2
    on = str(tmp_path / "on.vtk")
    ex.write_vtk(on)
    text = open(on, "rb").read()
    assert text.startswith(base)
    tok = text[len(base):].decode().split()
    assert tok[0] == "POINT_DATA" and int(tok[1]) == len(pc)
    back, at = parse_scalars(tok, 2, len(pc))
    assert back.tobytes() == pc.tobytes()
    assert tok[at] == "CELL_DATA" and int(tok[at + 1]) == len(cc)
    back, at = parse_scalars(tok, at + 2, len(cc))
    assert back.tobytes() == cc.tobytes() and at == len(tok)
    # off again: the bytes of a file written before the setter was ever called
    ex.set_components(False)
    ex.extract_host(vol, prm)
    off = str(tmp_path / "off.vtk")
    ex.write_vtk(off)
    assert open(off, "rb").read() == base
    # with normals and cell pixels: behind NORMALS in POINT_DATA, behind the pixels in CELL_DATA, the blocks not opened twice
    ex.set_point_normals(True)
    ex.set_cell_pixels(True)
    ex.extract_host(vol, prm)
    without = str(tmp_path / "without.vtk")
    ex.write_vtk(without)
    ex.set_components(True)
    ex.extract_host(vol, prm)
    both = str(tmp_path / "both.vtk")
    ex.write_vtk(both)
    a, b = open(without, "rb").read(), open(both, "rb").read()
    cut = a.index(b"CELL_DATA")
    assert b.startswith(a[:cut]) and b.count(b"POINT_DATA") == 1 and b.count(b"CELL_DATA") == 1
    tok = b[cut:].decode().split()
    back, at = parse_scalars(tok, 0, len(pc))
    assert back.tobytes() == pc.tobytes() and tok[at] == "CELL_DATA"
    tail = a[cut:].decode().split()
    assert tok[at:at + len(tail)] == tail
    back, at = parse_scalars(tok, at + len(tail), len(cc))
    assert back.tobytes() == cc.tobytes() and at == len(tok)
    ex.set_point_normals(False)
    ex.set_cell_pixels(False)


def test_python_filter_mirror(pkg):
    vox = cases.pair(0, 0, 2)
    f = pkg.CuberilleImageToMeshFilter(device=0)
    f.SetInput(pkg.Volume(vox))
    f.SetIsoSurfaceValue(1)
    f.Update()
    assert f.GetPointComponents() is None and f.GetNumberOfComponents() == 0 and not f.GetGenerateComponents()
    cells = f.GetOutput().cells
    f.GenerateComponentsOn()
    f.Update()
    assert f.GetGenerateComponents() and f.GetOutput().cells.tobytes() == cells.tobytes()
    want = ref.components(cells, len(f.GetOutput().points))
    same((f.GetPointComponents(), f.GetCellComponents(), f.GetComponentCellCounts()), want, "filter mirror")
    assert f.GetNumberOfComponents() == 2
    f.GenerateComponentsOff()
    f.Update()
    assert f.GetPointComponents() is None and f.GetNumberOfComponents() == 0
    g = pkg.CuberilleImageToMeshFilter(devices=[0, 0])
    g.SetInput(pkg.Volume(vox))
    g.SetIsoSurfaceValue(1)
    g.GenerateComponentsOn()
    with pytest.raises(Exception) as e:
        g.Update()
    assert "components" in str(e.value)


def test_drop_in_filter_components_update():
    """itk/tests/components_update.cxx: two balls are two components, and the filter's vectors equal a host union-find over the
    filled itk::Mesh's cells, with quads and with projected triangles; empty with the switch off -- the program exits non-zero on
    a difference."""
    exe = os.path.join(ROOT, "midas-journal-740_amd", "itk", "build", "components_update")
    if not os.path.exists(exe):
        pytest.fail("itk/build/components_update is missing: __graft_entry__.build() makes it")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout.strip(), run.stderr.strip())
    assert run.returncode == 0 and "GetNumberOfComponents() = 2" in run.stdout
    assert run.stdout.count("identical") == 3 and "DIFFERENT" not in run.stdout
