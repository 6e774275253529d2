"""cuberille_set_region on the GPU: the mesh of a box of a larger buffer, extracted in place.

The expected mesh is always the ORACLE's of the cropped copy -- np.ascontiguousarray(vol[z0:z1, y0:y1, x0:x1]) with the start
index moved by the box's place and the caller's origin / spacing / direction, what itk::ExtractImageFilter hands the reference
-- never the code under test.  Comparisons are exact: ids, order, float bits as uint32, cells, proj_iterations,
proj_stop_threshold, proj_stop_steps.  Only the default projection branch is used.

NaN coordinates (quirk Q4: a vertex whose gradient vanishes) are compared as bit patterns too, in two steps, because the sign
and payload of a NaN are the FPU's that made it -- the checker's come from the host, the library's from the GPU, region or no
region: a coordinate must be NaN in the oracle's mesh exactly where it is NaN in ours (every other coordinate: the oracle's
bits), and where both are NaN our bits must be those of the library's OWN extraction, region off, of the contiguous crop with
the moved start index -- the image the definition names.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from conftest import GOLDEN, ROOT
from gpu_helpers import _host_threads

pytestmark = pytest.mark.gpu

KW = dict(threshold=0.5, step=-1.0, relax=0.95, max_steps=50)
CASES = json.load(open(os.path.join(GOLDEN, "closed_border_cases.json")))["cases"]
PIXELS = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64, np.int64, np.uint64]
COUNTERS = ("proj_iterations", "proj_stop_threshold", "proj_stop_steps")
ARG = 1


def crop(vox, start, size):
    (x0, y0, z0), (nx, ny, nz) = start, size
    return np.ascontiguousarray(vox[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx])


def expected(oracle, vox, start, size, iso, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=None, s=(0, 0, 0), **kw):
    """The definition: the oracle on the cropped copy, its start index the input's plus the box's place."""
    box = crop(vox, start, size)
    at = tuple(int(a) + int(b) for a, b in zip(s, start))
    want = oracle.run(box, iso, spacing=spacing, origin=origin, direction=np.eye(3) if direction is None else direction,
                      index_start=at, **kw)

    def plain():
        """The library's own mesh of the contiguous crop, region off (only asked for where NaNs have to be compared)."""
        pkg = graft.load_package()
        e = pkg.Extractor(0)
        try:
            prm = pkg.make_params(iso, **{k: v for k, v in kw.items() if k != "gradient_threads"})
            e.extract_host(pkg.Volume(box, spacing, origin, direction, index_start=at), prm)
            return e.download()
        finally:
            e.close()
    want.plain = plain
    return want


def same(mesh, res, want, what=""):
    assert mesh.points.shape == want.points.shape and mesh.cells.shape == want.cells.shape, \
        (what, mesh.points.shape, want.points.shape, mesh.cells.shape, want.cells.shape)
    assert np.array_equal(mesh.cells, want.cells), (what, "cells differ")
    a, b = np.ascontiguousarray(mesh.points).view(np.uint32), np.ascontiguousarray(want.points).view(np.uint32)
    diff = a != b
    if diff.any():
        nan = np.isnan(mesh.points) & np.isnan(want.points)
        print(what, "%d coordinates differ from the oracle's bits, %d of them NaN in both; first %s: %08x / %08x" % (
            int(diff.sum()), int((diff & nan).sum()), np.argwhere(diff)[0], a[diff][0], b[diff][0]))
        assert not (diff & ~nan).any(), (what, "%d coordinates differ in their bits" % int((diff & ~nan).sum()))
        own = getattr(want, "plain", None)
        assert own is not None, (what, "NaN coordinates and no extraction of the crop to hold their bits to")
        p = np.ascontiguousarray(own().points).view(np.uint32)
        assert np.array_equal(a, p), (what, "%d coordinates differ from the library's own mesh of the crop" % int((a != p).sum()))
    if res is not None:
        assert {k: int(getattr(res, k)) for k in COUNTERS} == {k: want.info[k] for k in COUNTERS}, what


def routes(pkg, ex, vol, prm, which=("extract_device", "count + emit", "extract_host")):
    """(name, mesh, result) of the box through every whole-volume entry point; `vol` is the WHOLE buffer."""
    import torch
    desc = pkg.make_desc(vol.voxels.dtype, vol.dims, vol.spacing, vol.origin, vol.direction, vol.index_start)
    dev = torch.from_numpy(np.ascontiguousarray(vol.voxels).view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    if "extract_device" in which:
        res = ex.extract_device(dev.data_ptr(), desc, prm)
        yield "extract_device", ex.download(), res
    if "count + emit" in which:
        ex.count(dev.data_ptr(), desc, prm)
        res = ex.emit(0)
        yield "count + emit", ex.download(), res
    if "extract_host" in which:
        res = ex.extract_host(vol, prm)
        yield "extract_host", ex.download(), res


@pytest.fixture()
def ex(pkg):
    e = pkg.Extractor(0)
    yield e
    e.close()


def moved_central_half(n):
    """A box of the volume, off centre and at odd x: the central half, moved."""
    nx, ny, nz = n
    start = (nx // 4 + (1 - (nx // 4) % 2), ny // 4 + 1, nz // 4 - 1)
    return start, (nx // 2, ny // 2, nz // 2)


def box_cut_by_six_faces(inside):
    """The bounding box of the object drawn in by a quarter of its extent on every side (and to an odd x): the object crosses
    every one of its six faces."""
    start, size = [], []
    for ax in (2, 1, 0):                              # x, y, z of inside[z, y, x]
        w = np.flatnonzero(inside.any(axis=tuple(a for a in (0, 1, 2) if a != ax)))
        lo, hi = int(w[0]), int(w[-1]) + 1
        q = (hi - lo) // 4
        a, b = lo + q, hi - q
        if ax == 2 and a % 2 == 0 and b - a > 1:
            a += 1
        start.append(a)
        size.append(b - a)
    return tuple(start), tuple(size)


@pytest.mark.parametrize("case", CASES, ids=[c["input"] for c in CASES])
def test_reference_volumes_cut_by_all_six_faces(pkg, oracle, volumes, ex, case):
    """The reference's own volumes: a box the object crosses on all six faces (asserted), and the central half moved off
    centre: {triangles, quads} x {projection on, off} x every route, input start index zero and non-zero."""
    src = volumes(case["input"])
    whole = src.voxels >= case["iso"]
    cut = box_cut_by_six_faces(whole)
    inside = crop(whole, *cut)
    faces = [inside[0], inside[-1], inside[:, 0], inside[:, -1], inside[:, :, 0], inside[:, :, -1]]
    assert all(f.any() for f in faces), (case["input"], cut, [bool(f.any()) for f in faces])
    for start, size in (cut, moved_central_half(src.dims)):
        mixed = crop(whole, start, size)
        mixed = bool(mixed.any() and not mixed.all())         # (blob0 / blob1 are a voxel or two: their box is all inside)
        for s in ((0, 0, 0), (-7, 12, 100)):
            vol = pkg.Volume(src.voxels, src.spacing, src.origin, src.direction, index_start=s)
            for tri in (1, 0):
                for proj in (1, 0):
                    kw = dict(KW, triangles=tri, project=proj)
                    want = expected(oracle, src.voxels, start, size, case["iso"], src.spacing, src.origin, src.direction, s, **kw)
                    assert (len(want.cells) > 0) == mixed, (case["input"], start, size)
                    ex.set_region(start, size)
                    for name, mesh, res in routes(pkg, ex, vol, pkg.make_params(case["iso"], **kw)):
                        print(case["input"], start, size, s, tri, proj, name, mesh.points.shape, mesh.cells.shape)
                        same(mesh, res, want, (case["input"], start, size, s, tri, proj, name))


def field(n, dtype):
    """Inside values high, outside low, in the type's range; the object is larger than any box of it.  -> voxels, iso"""
    nx, ny, nz = n
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    r = np.sqrt(((x - nx * 0.47) / (nx * 0.5)) ** 2 + ((y - ny * 0.55) / (ny * 0.45)) ** 2 + ((z - nz * 0.5) / (nz * 0.5)) ** 2)
    f = np.clip(1.3 - r * 1.6 + 0.08 * np.sin(x * 1.7) * np.cos(y * 1.3 + z), 0.0, 1.0)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (f * 200.0 - 50.0).astype(dt), 37.5
    if dt.itemsize == 8:
        base = (1 << 62) if dt.kind == "u" else (1 << 61)
        vox = (np.floor(f * 200.0).astype(np.int64) + (base + 1)).astype(dt) if dt.kind == "i" else \
            (np.floor(f * 200.0).astype(np.uint64) + np.uint64(base + 1))
        return vox, base + 101                        # not a double: travels through iso_value_int
    span = min(int(np.iinfo(dt).max), 20000)
    return np.floor(f * span).astype(dt), span // 2


@pytest.mark.parametrize("dtype", PIXELS, ids=[np.dtype(d).name for d in PIXELS])
def test_all_pixel_types_both_sweeps(pkg, oracle, ex, dtype):
    """All ten pixel types, a box cut by all six faces inside a buffer with odd dims: the one-wave-per-word sweep (the default
    at this size) and the staged pitched spans (a development switch sends small boxes through them), every route."""
    vox, iso = field((83, 47, 29), dtype)
    vol = pkg.Volume(vox)
    start, size = (9, 5, 3), (41, 30, 21)
    for variant in (0, 2):
        ex.debug_option("classify_variant", variant)
        for proj in (1, 0):
            kw = dict(KW, triangles=1, project=proj)
            want = expected(oracle, vox, start, size, iso, **kw)
            assert len(want.cells) > 0
            ex.set_region(start, size)
            for name, mesh, res in routes(pkg, ex, vol, pkg.make_params(iso, **kw)):
                same(mesh, res, want, (np.dtype(dtype).name, variant, proj, name))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16], ids=["uint8", "int16"])
def test_every_residue_mod_16_bytes(pkg, oracle, ex, dtype):
    """1- and 2-byte pixels: box rows that start at every byte residue mod 16 (the buffer's rows are 101 voxels, so the residue
    also turns from row to row), boxes narrower than 64 voxels and wider, both sweeps -- the bit volume itself is compared."""
    import torch
    vox, iso = field((101, 23, 9), dtype)
    dev = torch.from_numpy(vox.view(np.uint8).reshape(-1)).cuda()
    desc = pkg.make_desc(vox.dtype, (101, 23, 9))
    prm = pkg.make_params(iso, **dict(KW, triangles=0, project=0))
    for x0 in range(16 // np.dtype(dtype).itemsize + 1):
        for nx in (37, 70):
            start, size = (x0, 2, 1), (nx, 17, 7)
            c = crop(vox, start, size)
            want_words = packed(c >= iso, nx)
            want = expected(oracle, vox, start, size, iso, **dict(KW, triangles=0, project=0))
            for variant in (0, 2):
                ex.debug_option("classify_variant", variant)
                ex.set_region(start, size)
                res = ex.extract_device(dev.data_ptr(), desc, prm)
                same(ex.download(), res, want, (x0, nx, variant))
                got = ex.debug_bits(size)
                assert np.array_equal(np.asarray(got).reshape(-1)[:want_words.size], want_words), (x0, nx, variant)


def packed(inside, nx):
    """The bit volume of a box as cuberille_debug_bits lays it out: (nx + 63) / 64 words a row, tail bits 0."""
    nz, ny, _ = inside.shape
    bits = np.zeros((nz, ny, (nx + 63) // 64 * 64), bool)
    bits[:, :, :nx] = inside
    return np.packbits(bits, axis=-1, bitorder="little").view("<u8").reshape(-1)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64], ids=["uint8", "int16", "float32", "float64"])
def test_staged_spans_that_begin_inside_a_row(pkg, oracle, ex, dtype):
    """The staged pitched spans over several spans whose first row is a partial one: boxes of more than 4096 words whose words
    per row (3, 5, 7) do not divide 4096, so that spans begin at word 1, 2, ... of a row, inside buffers whose row pitch is
    not a multiple of 16 bytes (the rows' skew to the 16-byte boundary turns from row to row and from span to span), and one
    whose slices are shorter than a span's rows (a span crosses slices).  The bit volume and the mesh against the oracle."""
    import torch
    for n, start, size in (((149, 47, 45), (7, 3, 2), (130, 40, 40)),       # W = 3: 4800 words, spans begin at words 1 and 2
                           ((331, 23, 61), (5, 2, 3), (300, 19, 55)),       # W = 5: 5225 words, slices of 95 words
                           ((449, 9, 133), (3, 1, 2), (420, 7, 128))):      # W = 7: 6272 words, a span crosses 83 slices
        assert (size[0] + 63) // 64 * size[1] * size[2] > 4096 and 4096 % ((size[0] + 63) // 64) != 0
        vox, iso = field(n, dtype)
        dev = torch.from_numpy(vox.view(np.uint8).reshape(-1)).cuda()
        desc = pkg.make_desc(vox.dtype, n, index_start=(2, -1, 5))
        want_words = packed(crop(vox, start, size) >= iso, size[0])
        for proj in (0, 1):
            kw = dict(KW, triangles=1, project=proj)
            want = expected(oracle, vox, start, size, iso, s=(2, -1, 5), **kw)
            assert len(want.cells) > 0
            for variant in (2, 0):
                ex.debug_option("classify_variant", variant)
                ex.set_region(start, size)
                res = ex.extract_device(dev.data_ptr(), desc, pkg.make_params(iso, **kw))
                got = np.asarray(ex.debug_bits(size)).reshape(-1)
                bad = np.flatnonzero(got != want_words)
                assert bad.size == 0, (np.dtype(dtype).name, n, variant, "%d words differ, first %d" % (bad.size, bad[0]))
                same(ex.download(), res, want, (np.dtype(dtype).name, n, variant, proj))


def test_row_shapes_and_thin_crops(pkg, oracle, ex):
    """Box rows that are not whole words inside buffers that are, and the reverse; z-only, y-only and x-only crops (the first
    is contiguous in memory: a pointer offset); the smallest box; through both sweeps."""
    for n, start, size in (((192, 20, 12), (31, 3, 2), (130, 12, 8)),        # ragged box, whole-word buffer
                           ((150, 20, 12), (11, 3, 2), (128, 12, 8)),        # whole-word box, ragged buffer
                           ((128, 20, 12), (0, 0, 3), (128, 20, 7)),         # z only
                           ((128, 20, 12), (0, 5, 0), (128, 9, 12)),         # y only
                           ((128, 20, 12), (33, 0, 0), (64, 20, 12)),        # x only
                           ((70, 20, 12), (35, 10, 6), (1, 1, 1)),           # the smallest box
                           ((70, 20, 12), (35, 10, 6), (2, 1, 3))):
        vox, iso = field(n, np.float32)
        vol = pkg.Volume(vox, index_start=(3, 0, -2))
        for variant in (0, 2):
            ex.debug_option("classify_variant", variant)
            kw = dict(KW, triangles=1, project=1)
            want = expected(oracle, vox, start, size, iso, s=(3, 0, -2), **kw)
            ex.set_region(start, size)
            for name, mesh, res in routes(pkg, ex, vol, pkg.make_params(iso, **kw)):
                same(mesh, res, want, (n, start, size, variant, name))


def test_whole_buffer_box_equals_region_off(pkg, oracle, ex):
    vox, iso = field((70, 33, 17), np.float32)
    vol = pkg.Volume(vox, spacing=(0.7, 0.7, 2.5), index_start=(4, 5, 6))
    prm = pkg.make_params(iso, **dict(KW, triangles=1, project=1))
    ex.extract_host(vol, prm)
    off = ex.download()
    want = oracle.run(vox, iso, spacing=(0.7, 0.7, 2.5), index_start=(4, 5, 6), **dict(KW, triangles=1, project=1))
    ex.set_region((0, 0, 0), (70, 33, 17))
    for name, mesh, res in routes(pkg, ex, vol, prm):
        same(mesh, res, want, name)
        assert mesh.points.tobytes() == off.points.tobytes() and mesh.cells.tobytes() == off.cells.tobytes()


ROT = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
TILT = np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]])


@pytest.mark.parametrize("geom", ["identity", "axis-aligned", "rotated", "tilted"])
def test_three_geometry_forms(pkg, oracle, ex, geom):
    """Identity, axis-aligned (any spacing) and general geometry, input start index zero and non-zero, origin off zero."""
    spacing, direction = {"identity": ((1.0, 1.0, 1.0), np.eye(3)), "axis-aligned": ((0.7, 0.7, 2.5), np.eye(3)),
                          "rotated": ((0.7, 0.9, 1.3), ROT), "tilted": ((1.1, 0.9, 1.3), TILT)}[geom]
    vox, iso = field((90, 41, 25), np.float32)
    start, size = (13, 6, 4), (66, 30, 17)
    for s in ((0, 0, 0), (100, -20, 7)):
        for origin in ((0.0, 0.0, 0.0), (-3.5, 10.25, 0.125)):
            vol = pkg.Volume(vox, spacing, origin, direction, index_start=s)
            for tri in (1, 0):
                kw = dict(KW, triangles=tri, project=1)
                want = expected(oracle, vox, start, size, iso, spacing, origin, direction, s, **kw)
                ex.set_region(start, size)
                for name, mesh, res in routes(pkg, ex, vol, pkg.make_params(iso, **kw)):
                    same(mesh, res, want, (geom, s, origin, tri, name))


def test_quirk_q1_inside_a_box(pkg, oracle, ex):
    """Empty slices between occupied ones inside the box (the reference re-uses the vertices of the last occupied slice)."""
    vox = np.zeros((20, 24, 40), np.uint8)
    vox[3:5, 4:15, 6:30] = 200
    vox[9:12, 6:18, 10:33] = 200
    vox[14, 2:20, 3:36] = 200
    vox[18:, :, :] = 200                              # outside the box: must not matter
    vol = pkg.Volume(vox)
    start, size = (5, 3, 2), (29, 18, 15)
    for tri in (1, 0):
        kw = dict(KW, triangles=tri, project=1)
        want = expected(oracle, vox, start, size, 100, **kw)
        ex.set_region(start, size)
        for name, mesh, res in routes(pkg, ex, vol, pkg.make_params(100, **kw)):
            same(mesh, res, want, (tri, name))
    occ = np.asarray(ex.slice_occupancy(size[2]))
    assert occ.tolist() == [int(crop(vox, start, size)[z].max() >= 100) for z in range(size[2])]


def test_extract_host_through_the_chunk_pipeline(pkg, oracle, ex):
    """The host route above the chunking threshold's code path (a development switch sends a small image through the pipeline in
    chunks of a few slices): the staging threads gather the box's rows; a z-only box takes the pipeline's plain copy."""
    vox, iso = field((200, 120, 64), np.float32)
    vol = pkg.Volume(vox, index_start=(1, 2, 3))
    kw = dict(KW, triangles=1, project=1)
    for start, size in (((21, 9, 5), (150, 100, 50)), ((0, 0, 7), (200, 120, 40))):
        want = expected(oracle, vox, start, size, iso, s=(1, 2, 3), **kw)
        ex.set_region(start, size)
        for kib in (0, 256, 64):
            ex.debug_option("upload_chunk_kib", kib)
            res = ex.extract_host(vol, pkg.make_params(iso, **kw))
            same(ex.download(), res, want, (start, size, kib))
    ex.debug_option("upload_chunk_kib", 0)
    ex.clear_region()
    ex.debug_option("upload_chunk_kib", 128)          # ... and the pipeline without a region, as before
    res = ex.extract_host(vol, pkg.make_params(iso, **kw))
    same(ex.download(), res, oracle.run(vox, iso, index_start=(1, 2, 3), **kw), "no region, chunked")


def big_sphere(shape, centre, radius, dtype, device):
    import torch
    nz, ny, nx = shape
    z = torch.arange(nz, device=device, dtype=torch.float32).view(-1, 1, 1)
    y = torch.arange(ny, device=device, dtype=torch.float32).view(1, -1, 1)
    x = torch.arange(nx, device=device, dtype=torch.float32).view(1, 1, -1)
    f = radius - torch.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    if dtype == np.uint8:
        return torch.clamp(f * 4.0 + 128.0, 0, 255).to(torch.uint8)
    return f


@pytest.mark.parametrize("dtype,buf,start,size", [(np.float32, (1100, 1060, 270), (37, 21, 5), (1024, 1024, 256)),
                                                  (np.uint8, (1111, 1037, 170), (55, 13, 7), (1000, 1000, 160))],
                         ids=["f32-1024x1024x256", "u8-1000x1000x160"])
def test_production_launch_shapes(pkg, oracle, ex, dtype, buf, start, size):
    """Production launch shapes inside larger buffers, a sphere the box cuts on every face.  The float32 box (1 GiB) takes the
    staged pitched spans and the refilling walk by the default rules; the uint8 box (160 MB, under the 256 MiB rule) takes the
    one-wave-per-word sweep by default and is sent through the staged spans once more by the development switch -- 1-byte
    pixels have the largest stage and every byte alignment (its rows lie 1111 bytes apart)."""
    import torch
    Nx, Ny, Nz = buf
    dev = big_sphere((Nz, Ny, Nx), (start[0] + size[0] * 0.5, start[1] + size[1] * 0.52, start[2] + size[2] * 0.45),
                     0.56 * size[0], dtype, "cuda")
    host = dev.cpu().numpy()
    iso = 0.0 if dtype == np.float32 else 128
    kw = dict(triangles=1, project=1, threshold=0.05, step=0.25, relax=0.95, max_steps=50)
    desc = pkg.make_desc(dtype, buf, index_start=(3, 2, 1))
    want = expected(oracle, host, start, size, iso, s=(3, 2, 1), gradient_threads=_host_threads(), **kw)
    assert len(want.points) > 100000
    ex.set_region(start, size)
    torch.cuda.synchronize()
    for _ in range(2):              # the second extraction on a context launches blindly, sized by the first
        res = ex.extract_device(dev.data_ptr(), desc, pkg.make_params(iso, **kw))
        same(ex.download(), res, want, "extract_device")
    ex.count(dev.data_ptr(), desc, pkg.make_params(iso, **kw))
    res = ex.emit(0)
    same(ex.download(), res, want, "count + emit")
    if dtype == np.uint8:
        ex.debug_option("classify_variant", 2)
        res = ex.extract_device(dev.data_ptr(), desc, pkg.make_params(iso, **kw))
        same(ex.download(), res, want, "extract_device, staged spans")
        words = np.asarray(ex.debug_bits(size)).reshape(-1)
        assert np.array_equal(words, packed(crop(host, start, size) >= iso, size[0]))


def test_no_state_leaks_and_warm_up_reserves_the_box(pkg, oracle, ex):
    """Region on -> off -> another box on one context; warm_up with a region reserves the box's sizes, not the buffer's."""
    import torch
    vox, iso = field((90, 41, 25), np.float32)
    vol = pkg.Volume(vox)
    kw = dict(KW, triangles=1, project=1)
    prm = pkg.make_params(iso, **kw)
    for box in (((13, 6, 4), (66, 30, 17)), None, ((1, 0, 2), (30, 41, 9)), None, ((40, 20, 10), (50, 21, 15))):
        if box is None:
            ex.clear_region()
            want = oracle.run(vox, iso, **kw)
        else:
            ex.set_region(*box)
            want = expected(oracle, vox, box[0], box[1], iso, **kw)
        for name, mesh, res in routes(pkg, ex, vol, prm):
            same(mesh, res, want, (box, name))
    # warm_up: a 64^3 box of a 1024 x 512 x 512 float buffer reserves nothing the size of the buffer (2^30 bytes)
    e = pkg.Extractor(0)
    try:
        e.warm_up()
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        e.set_region((100, 100, 100), (64, 64, 64))
        e.warm_up(pkg.make_desc(np.float32, (1024, 512, 512)))
        torch.cuda.synchronize()
        used = before - torch.cuda.mem_get_info()[0]
        print("warm_up with a 64^3 box of a 1 GiB buffer reserved", used, "bytes")
        assert used < (64 << 20)
        with pytest.raises(pkg._abi.CuberilleError):          # ... and reports a box that leaves the buffer it is told of
            e.warm_up(pkg.make_desc(np.float32, (128, 128, 128)))
    finally:
        e.close()


def test_every_refusal_then_a_plain_extraction(pkg, oracle, ex):
    import torch
    vox, iso = field((40, 30, 20), np.float32)
    vol = pkg.Volume(vox)
    desc = pkg.make_desc(np.float32, (40, 30, 20))
    dev = torch.from_numpy(vox.reshape(-1)).cuda()
    torch.cuda.synchronize()
    kw = dict(KW, triangles=1, project=1)
    prm = pkg.make_params(iso, **kw)
    L, ctx = ex._lib, ex._ctx

    def refused(fn, code=ARG):
        with pytest.raises(pkg._abi.CuberilleError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        assert "region" in str(e.value)

    def plain():
        ex.clear_region()
        ex.set_border(0, 0)
        ex.hold_gradient(False)
        ex.set_interpolator(pkg._abi.INTERP_LINEAR)
        ex.extract_host(vol, prm)
        same(ex.download(), ex.result, oracle.run(vox, iso, **kw), "plain")

    import ctypes as C
    bad = (C.c_int64 * 3)(-1, 0, 0)
    five = (C.c_int64 * 3)(5, 5, 5)
    zero = (C.c_int64 * 3)(0, 0, 0)
    ex.set_region((1, 2, 3), (10, 9, 8))
    assert L.cuberille_set_region(ctx, bad, five) == ARG          # negative start, non-positive size: the setting stays
    assert L.cuberille_set_region(ctx, zero, (C.c_int64 * 3)(5, 0, 5)) == ARG
    assert L.cuberille_set_region(ctx, zero, None) == ARG
    res = ex.extract_host(vol, prm)
    same(ex.download(), res, expected(oracle, vox, (1, 2, 3), (10, 9, 8), iso, **kw), "setting unchanged")
    # a box that leaves THIS buffer: at the extraction, every route (the raw calls: the Python mirror checks earlier)
    start, size = (C.c_int64 * 3)(35, 0, 0), (C.c_int64 * 3)(10, 9, 8)
    assert L.cuberille_set_region(ctx, start, size) == 0
    r = pkg._abi.Result()
    assert L.cuberille_extract_device(ctx, C.byref(desc), C.c_void_p(dev.data_ptr()), C.byref(prm), None, C.byref(r)) == ARG
    assert L.cuberille_extract_host(ctx, C.byref(desc), C.c_void_p(vox.ctypes.data), C.byref(prm), C.byref(r)) == ARG
    n1, n2 = C.c_uint64(), C.c_uint64()
    assert L.cuberille_count(ctx, C.byref(desc), C.c_void_p(dev.data_ptr()), C.byref(prm), None, C.byref(n1), C.byref(n2)) == ARG
    plain()
    box = ((1, 2, 3), (10, 9, 8))
    # a slab that is not the whole volume
    ex.set_region(*box)
    slab = pkg._abi.Slab(global_nz=40, z_begin=10, own_z0=12, own_z1=20)
    refused(lambda: ex.extract_device(dev.data_ptr(), desc, prm, slab))
    refused(lambda: ex.count(dev.data_ptr(), desc, prm, slab))
    # the step calls, the stream
    refused(lambda: ex.step_begin(dev.data_ptr(), desc, prm))
    refused(lambda: ex.step_classify(dev.data_ptr(), desc, prm))
    refused(lambda: ex.extract_stream(desc, lambda dst, z0, z1: None, prm))
    plain()
    # together with an implied border
    ex.set_region(*box)
    ex.set_border(1, 0)
    refused(lambda: ex.extract_host(vol, prm))
    refused(lambda: ex.extract_device(dev.data_ptr(), desc, prm))
    plain()
    # with project_vertices on: B-spline, held gradient, recursive Gaussian, the two projection branches
    ex.set_region(*box)
    ex.set_interpolator(pkg._abi.INTERP_BSPLINE, 3, 32, 32)
    refused(lambda: ex.extract_host(vol, prm))
    ex.set_interpolator(pkg._abi.INTERP_LINEAR)
    ex.hold_gradient(True)
    refused(lambda: ex.extract_host(vol, prm))
    ex.hold_gradient(False)
    refused(lambda: ex.extract_host(vol, pkg.make_params(iso, gradient=1, **kw)))
    refused(lambda: ex.extract_host(vol, pkg.make_params(iso, variant=1, **kw)))
    refused(lambda: ex.extract_host(vol, pkg.make_params(iso, variant=2, **kw)))
    # ... and with the projection off those settings do not matter
    res = ex.extract_host(vol, pkg.make_params(iso, gradient=1, **dict(kw, project=0)))
    same(ex.download(), res, expected(oracle, vox, box[0], box[1], iso, **dict(kw, project=0)), "no projection")
    plain()
    # a group with a member that has a region
    g = pkg.ExtractorGroup([0, 0])
    try:
        g.set_region(*box)
        with pytest.raises(pkg._abi.CuberilleError) as e:
            g.extract_host(vol, prm)
        assert e.value.code == ARG and "region" in str(e.value)
        g.set_region((0, 0, 0), (0, 0, 0))
        g.extract_host(vol, prm)
        same(g.download(), None, oracle.run(vox, iso, **kw), "group, region off")
    finally:
        g.close()
    plain()


def test_no_copy_of_the_voxels(pkg, ex):
    """Free device memory around a region extract_device after warm_up: a float32 box against a uint8 box of equal size inside
    equal buffers -- what the two reserve may differ by nothing that scales with sizeof(pixel) * box: less than one eighth
    of the float box's voxels (a cropped copy would be 8/8 of them against 2/8)."""
    import torch
    N, start, size = 640, (64, 32, 16), (512, 512, 512)
    used = {}
    for dt in (np.float32, np.uint8):
        dev = big_sphere((N, N, N), (320.0, 300.0, 280.0), 230.0, dt, "cuda")
        torch.cuda.synchronize()
        e = pkg.Extractor(0)
        try:
            e.warm_up()
            torch.cuda.synchronize()
            before = torch.cuda.mem_get_info()[0]
            e.set_region(start, size)
            desc = pkg.make_desc(dt, (N, N, N))
            prm = pkg.make_params(0.0 if dt == np.float32 else 128, **dict(KW, triangles=1, project=1))
            e.extract_device(dev.data_ptr(), desc, prm)
            torch.cuda.synchronize()
            used[dt] = before - torch.cuda.mem_get_info()[0]
            assert int(e.result.n_points) > 100000
        finally:
            e.close()
        del dev
    voxel_bytes = 512 ** 3 * 4
    print("device bytes reserved: float32 box %d, uint8 box %d, float32 box's voxels %d" % (used[np.float32], used[np.uint8], voxel_bytes))
    assert abs(used[np.float32] - used[np.uint8]) < voxel_bytes // 8


def test_equals_the_library_on_torch_contiguous(pkg, ex):
    """Not through the oracle: the region extraction equals the library's own extraction of torch's .contiguous() of the same
    view with the moved start index -- bytes and counters."""
    import torch
    vox, iso = field((150, 90, 70), np.float32)
    dev = torch.from_numpy(vox).cuda()
    start, size = (17, 9, 5), (120, 70, 60)
    view = dev[start[2]:start[2] + size[2], start[1]:start[1] + size[1], start[0]:start[0] + size[0]].contiguous()
    torch.cuda.synchronize()
    for spacing in ((1.0, 1.0, 1.0), (0.7, 0.7, 2.5)):
        prm = pkg.make_params(iso, **dict(KW, triangles=1, project=1))
        ex.clear_region()
        a = ex.extract_device(view.data_ptr(), pkg.make_desc(np.float32, size, spacing=spacing, index_start=(17 + 4, 9 - 3, 5 + 11)), prm)
        ma = ex.download()
        ca = {k: int(getattr(a, k)) for k in COUNTERS}
        ex.set_region(start, size)
        b = ex.extract_device(dev.data_ptr(), pkg.make_desc(np.float32, (150, 90, 70), spacing=spacing, index_start=(4, -3, 11)), prm)
        mb = ex.download()
        assert ma.points.tobytes() == mb.points.tobytes() and ma.cells.tobytes() == mb.cells.tobytes()
        assert ca == {k: int(getattr(b, k)) for k in COUNTERS}
        assert len(ma.points) > 1000


def test_python_filter_mirror(pkg, oracle):
    vox, iso = field((60, 40, 30), np.float32)
    s = (10, -5, 3)
    vol = pkg.Volume(vox, spacing=(0.7, 0.7, 2.5), index_start=s)
    f = pkg.CuberilleImageToMeshFilter(device=0)
    f.SetInput(vol)
    f.SetIsoSurfaceValue(iso)
    f.SetExtractionRegion((10 + 7, -5 + 4, 3 + 2), (40, 30, 20))
    f.Update()
    want = expected(oracle, vox, (7, 4, 2), (40, 30, 20), iso, spacing=(0.7, 0.7, 2.5), s=s)
    same(f.GetOutput(), f.last_result, want, "filter")
    f.SetExtractionRegion((9, -5, 3), (40, 30, 20))               # an index below the input's
    with pytest.raises(pkg._abi.CuberilleError):
        f.Update()
    f.ClearExtractionRegion()
    f.Update()
    same(f.GetOutput(), f.last_result, oracle.run(vox, iso, spacing=(0.7, 0.7, 2.5), index_start=s), "filter, region cleared")


def test_drop_in_filter_region_update(pkg, volumes, tmp_path):
    """itk/tests/region_update.cxx: Update() with SetExtractionRegion on the big image against Update() on the hand-made crop
    whose region keeps the index -- the program exits non-zero on a difference -- and a box outside the buffered region."""
    exe = os.path.join(ROOT, "midas-journal-740_amd", "itk", "build", "region_update")
    if not os.path.exists(exe):
        pytest.fail("itk/build/region_update is missing: __graft_entry__.build() makes it")
    for name, iso in (("nucleon.mha", 140), ("silicium.mha", 85)):
        src = volumes(name)
        start, size = box_cut_by_six_faces(src.voxels >= iso)
        path = os.path.join(GOLDEN, "data", name)
        for tri, s in (("1", (0, 0, 0)), ("0", (5, -3, 40))):
            args = [exe, path, str(iso)] + [str(a + b) for a, b in zip(start, s)] + [str(v) for v in size] + [tri] + [str(v) for v in s]
            run = subprocess.run(args, capture_output=True, text=True, timeout=300)
            print(run.stdout.strip(), run.stderr.strip())
            assert run.returncode == 0 and "identical" in run.stdout
    args = [exe, os.path.join(GOLDEN, "data", "nucleon.mha"), "140", "-1", "0", "0", "5", "5", "5"]
    run = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 3 and "buffered region" in run.stderr
