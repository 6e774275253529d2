"""Python host side of the MI355X cuberille path.

`CuberilleImageToMeshFilter` mirrors the public surface of the reference class
(/root/reference/Source/itkCuberilleImageToMeshFilter.h:180-228: the same
Set/Get names, defaults of txx:33-40, clamps of h:210,216,223, On/Off helpers,
Update()/GetOutput()) so the parity tests read like the reference's own driver
(/root/reference/Testing/CuberilleTest01.cxx:144-162).  `Extractor` is the thin
layer over the C ABI (include/cuberille_hip.h) used by bench.py and the multi-GPU
driver.  Everything computes on the GPU through libcuberille_hip.so; nothing here
falls back to a CPU implementation.
"""
import collections
import ctypes as C
import math
import os

import numpy as np

from . import _abi
from .mha import Volume

PIXEL_CODES = {
    np.dtype(np.uint8): 0, np.dtype(np.int8): 1, np.dtype(np.uint16): 2, np.dtype(np.int16): 3,
    np.dtype(np.uint32): 4, np.dtype(np.int32): 5, np.dtype(np.float32): 6, np.dtype(np.float64): 7,
    np.dtype(np.int64): 8, np.dtype(np.uint64): 9,
}
PIXEL_DTYPES = {code: dt for dt, code in PIXEL_CODES.items()}


def _torch():
    import torch
    return torch


_TORCH_TO_NP = None


def _np_dtype_of(t):
    global _TORCH_TO_NP
    torch = _torch()
    if _TORCH_TO_NP is None:
        _TORCH_TO_NP = {torch.uint8: np.uint8, torch.int8: np.int8, torch.int16: np.int16, torch.int32: np.int32,
                        torch.int64: np.int64, torch.float32: np.float32, torch.float64: np.float64}
        for name, npd in (("uint16", np.uint16), ("uint32", np.uint32), ("uint64", np.uint64)):
            if hasattr(torch, name):
                _TORCH_TO_NP[getattr(torch, name)] = npd
    return np.dtype(_TORCH_TO_NP[t.dtype])


class Mesh:
    """Flat mesh: points float32 [n,3]; cells uint64 [m,3|4] of GLOBAL point ids."""

    def __init__(self, points, cells, point_id_offset=0):
        self.points = points
        self.cells = cells
        self.point_id_offset = point_id_offset

    def GetNumberOfPoints(self):
        return int(self.points.shape[0])

    def GetNumberOfCells(self):
        return int(self.cells.shape[0])

    def write_vtk(self, path, threads=0):
        """Legacy-ASCII VTK POLYDATA straight from the flat buffers (include/cuberille_hip.h:
        cuberille_write_vtk_buffers), the bytes itk::VTKPolyDataWriter gives at CuberilleTest01.cxx:180-187."""
        pts = np.ascontiguousarray(self.points, dtype=np.float32)
        cells = np.ascontiguousarray(self.cells, dtype=np.uint64)
        rc = _abi.lib().cuberille_write_vtk_buffers(os.fsencode(path), C.c_void_p(pts.ctypes.data), pts.shape[0],
                                                    C.c_void_p(cells.ctypes.data), cells.shape[0],
                                                    int(cells.shape[1]) if cells.ndim == 2 else 3, int(threads))
        if rc != _abi.OK:
            raise _abi.CuberilleError(rc, "cannot write %s" % path)


SlabInfo = collections.namedtuple("SlabInfo", "alias_below lowest highest second_highest alias_z")

PROJECT_DEFAULT, PROJECT_ADVANCED, PROJECT_LINESEARCH = 0, 1, 2    # include/cuberille_hip.h CUBERILLE_PROJECT_*


GRADIENT_CENTRAL, GRADIENT_RECURSIVE_GAUSSIAN = 0, 1               # include/cuberille_hip.h CUBERILLE_GRADIENT_*


def make_params(iso, triangles=True, project=True, threshold=0.5, step=-1.0, relax=0.95, max_steps=50, q1=True,
                variant=PROJECT_DEFAULT, gradient=GRADIENT_CENTRAL):
    """variant picks the branch of ProjectVertexToIsoSurface: the shipped one (txx:439-474) or one of the two the
    reference compiles out (USE_ADVANCED_PROJECTION txx:340-397, USE_LINESEARCH_PROJECTION txx:398-437; h:22-23).
    gradient: the shipped central differences, or USE_GRADIENT_RECURSIVE_GAUSSIAN (h:21; txx:488-491; parity unpinned)."""
    # The 64-bit integer pixel types take the iso value as an integer (a double cannot hold it past 2^53): converted like
    # the C cast the reference makes of it (m_IsoSurfaceValue IS an InputPixelType, h:180-181), i.e. truncated toward
    # zero -- 100.5 is 100, as for every other integer pixel type.  A value no 64-bit type can hold (NaN, an infinity,
    # beyond -2^63 .. 2^64 - 1) leaves `iso_int_exact` None, and the entry points refuse it for those pixel types.
    exact = iso_int_of(iso)
    iso_int = 0 if exact is None else ((exact + (1 << 63)) % (1 << 64)) - (1 << 63)   # uint64 above 2^63: the same 64 bits
    prm = _abi.Params(float(iso), int(bool(triangles)), int(bool(project)), float(threshold), float(step),
                      float(relax), int(max_steps), int(bool(q1)), int(variant), int(gradient), iso_int)
    prm.iso_int_exact = exact
    return prm


def iso_int_of(iso):
    """The iso value as the integer a C cast to a 64-bit integer pixel type gives: truncated toward zero; None when no
    such type holds it."""
    try:
        v = int(iso) if isinstance(iso, (int, np.integer)) else math.trunc(float(iso))
    except (OverflowError, ValueError):          # inf, NaN
        return None
    return v if -(1 << 63) <= v < (1 << 64) else None


def check_iso(pixel_type, params):
    """64-bit integer pixels: the iso value must be one the pixel type holds (the other integer types are range-checked
    by the library against iso_value itself).  Parameters not made by make_params are taken as they are."""
    if pixel_type not in (8, 9) or not hasattr(params, "iso_int_exact"):
        return
    v = params.iso_int_exact
    lo, hi = (-(1 << 63), 1 << 63) if pixel_type == 8 else (0, 1 << 64)
    if v is None or not (lo <= v < hi):
        raise _abi.CuberilleError(_abi.ERR_ARGUMENT, "iso value is not representable in the pixel type")


def check_border(pixel_type, border):
    """64-bit integer pixels: the border value of Extractor.set_border must be one the pixel type holds (the library checks
    the other integer types itself, as it does the iso value)."""
    if pixel_type not in (8, 9) or not border or not border[0]:
        return
    v = border[1]
    lo, hi = (-(1 << 63), 1 << 63) if pixel_type == 8 else (0, 1 << 64)
    if v is None or not (lo <= v < hi):
        raise _abi.CuberilleError(_abi.ERR_ARGUMENT, "the border value is not representable in the pixel type")


def _band_arrays(band):
    """(lower, upper, inside, outside) as the two arrays cuberille_set_band / cuberille_band_check take: doubles, and the
    64 bits a 64-bit integer pixel type would hold (a uint64 past 2^63 wraps, like the iso value)."""
    exact = [iso_int_of(x) for x in band]
    v = (C.c_double * 4)(*[float(x) for x in band])
    vi = (C.c_int64 * 4)(*[0 if e is None else ((e + (1 << 63)) % (1 << 64)) - (1 << 63) for e in exact])
    return v, vi, exact


def check_band(pixel_type, band):
    """(lower, upper, inside, outside) of Extractor.set_band against a pixel type (cuberille_band_check, no GPU): raises what
    the library would at the extraction -- ERR_ARGUMENT for a value the pixel type does not hold (outside its range, or a
    fraction for an integer type), for lower > upper and for a NaN bound.  band None: nothing to check."""
    if band is None:
        return
    v, vi, exact = _band_arrays(band)
    if int(pixel_type) in (8, 9):
        # (the library judges the range of the 64-bit integer types by the double; a Python integer says it exactly)
        lo, hi = (-(1 << 63), 1 << 63) if int(pixel_type) == 8 else (0, 1 << 64)
        for e in exact:
            if e is None or not (lo <= e < hi):
                raise _abi.CuberilleError(_abi.ERR_ARGUMENT, "band (cuberille_set_band): a value is not representable in the pixel type")
    rc = _abi.lib().cuberille_band_check(int(pixel_type), v, vi)
    if rc:
        text = _abi.lib().cuberille_last_error(None)      # (the library's own words, kept per thread)
        raise _abi.CuberilleError(rc, text.decode() if text else "")


def region_desc(desc, start_xyz, size_xyz):
    """The description of the box [start, start + size) of the buffer `desc` describes (cuberille_region_desc, no GPU): dims
    = size, index_start = the buffer's + start, the same origin, spacing and direction -- the image
    itk::ExtractImageFilter would hand the reference, its index kept.  start is a position in the buffer (x, y, z).  Raises
    CuberilleError: ERR_ARGUMENT for a negative start, an empty size or a box that leaves the buffer, ERR_LIMIT where the
    box's start index leaves +-2^30 or start index + size exceeds 2^31 - 1.  size (0, 0, 0): the buffer itself."""
    out = _abi.ImageDesc()
    start = (C.c_int64 * 3)(*[int(v) for v in start_xyz])
    size = (C.c_int64 * 3)(*[int(v) for v in size_xyz])
    rc = _abi.lib().cuberille_region_desc(C.byref(desc), start, size, C.byref(out))
    if rc:
        text = _abi.lib().cuberille_last_error(None)      # (the library's own words, kept per thread)
        raise _abi.CuberilleError(rc, text.decode() if text else "")
    return out


def check_region(desc, region):
    """The box of Extractor.set_region against the buffer an extraction is about to be handed: raises what the library
    would (region_desc), before a device is touched.  region: None, or (start_xyz, size_xyz)."""
    if region is not None:
        region_desc(desc, region[0], region[1])


def make_desc(np_dtype, dims_xyz, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=None, index_start=(0, 0, 0)):
    d = _abi.ImageDesc()
    d.pixel_type = PIXEL_CODES[np.dtype(np_dtype)]
    d.dims[:] = [int(v) for v in dims_xyz]
    d.spacing[:] = [float(v) for v in spacing]
    d.origin[:] = [float(v) for v in origin]
    dm = np.eye(3) if direction is None else np.asarray(direction, dtype=np.float64)
    d.direction[:] = [float(v) for v in dm.reshape(9)]
    d.index_start[:] = [int(v) for v in index_start]        # (x, y, z) of GetBufferedRegion().GetIndex(); 0 for files
    return d


def _set_point_scalars(lib, ctx, image, outside):
    """cuberille_set_point_scalars on one context; image: a Volume (host), a (dev_ptr, desc) pair (device) or None (off)."""
    if image is None:
        _abi.check(ctx, lib.cuberille_set_point_scalars(ctx, None, None, 0, 0.0))
    elif isinstance(image, tuple):
        dev_ptr, desc = image
        _abi.check(ctx, lib.cuberille_set_point_scalars(ctx, C.byref(desc), C.c_void_p(dev_ptr), _abi.MEM_DEVICE, float(outside)))
    else:
        vox = np.ascontiguousarray(image.voxels)
        desc = make_desc(vox.dtype, image.dims, image.spacing, image.origin, image.direction, getattr(image, "index_start", (0, 0, 0)))
        _abi.check(ctx, lib.cuberille_set_point_scalars(ctx, C.byref(desc), C.c_void_p(vox.ctypes.data), _abi.MEM_HOST, float(outside)))


class Extractor:
    """One context (stream + workspace) on one GPU."""

    def __init__(self, device=0):
        self._lib = _abi.lib()
        self._ctx = C.c_void_p()
        rc = self._lib.cuberille_create(C.byref(self._ctx), int(device))
        if rc != _abi.OK:
            text = self._lib.cuberille_last_error(None)
            self._ctx = C.c_void_p()
            raise _abi.CuberilleError(rc, text.decode() if text else "")
        self.device = int(device)
        self.result = None
        # what the view setters left: border (width, the value as a 64-bit integer pixel type would hold it), region
        # ((start_xyz, size_xyz) of the box, or None), band ((lower, upper, inside, outside), or None)
        self._view = {"border": (0, 0), "region": None, "band": None}

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.cuberille_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_view(self, desc, params, boxed=True):
        """What can be said of the iso value and of the view settings (set_border, set_region) against the image an entry
        point is about to be handed, before a device is touched; the library says the rest, the band's part included.
        boxed: the entry point offers a region, so a box is held against desc; the others leave a set region to the
        library's refusal."""
        check_iso(int(desc.pixel_type), params)
        check_border(int(desc.pixel_type), self._view["border"])
        if boxed:
            check_region(desc, self._view["region"])

    def warm_up(self, desc=None, params=None):
        """cuberille_warm_up: load the code objects and, with an image description, reserve the workspace for such a volume
        -- what the first extraction on a fresh context would otherwise pay inside its own call."""
        _abi.check(self._ctx, self._lib.cuberille_warm_up(self._ctx, C.byref(desc) if desc is not None else None,
                                                          C.byref(params) if params is not None else None))

    def use_torch_stream(self):
        """Order this context's work on torch's current stream."""
        torch = _torch()
        s = torch.cuda.current_stream(self.device).cuda_stream
        _abi.check(self._ctx, self._lib.cuberille_set_stream(self._ctx, C.c_void_p(s)))

    def use_stream(self, torch_stream):
        """Order this context's work on a torch.cuda.Stream of the caller's."""
        _abi.check(self._ctx, self._lib.cuberille_set_stream(self._ctx, C.c_void_p(torch_stream.cuda_stream)))

    def use_own_stream(self):
        """Back to the context's own stream (the default)."""
        _abi.check(self._ctx, self._lib.cuberille_set_stream(self._ctx, C.c_void_p(0)))

    # -- whole-path entry points -----------------------------------------------------------
    def extract_host(self, vol, params):
        """vol: mha.Volume in host memory.  Upload + extract (PCIe-inclusive)."""
        vox = np.ascontiguousarray(vol.voxels)
        desc = make_desc(vox.dtype, vol.dims, vol.spacing, vol.origin, vol.direction, getattr(vol, "index_start", (0, 0, 0)))
        self._check_view(desc, params)
        res = _abi.Result()
        _abi.check(self._ctx, self._lib.cuberille_extract_host(
            self._ctx, C.byref(desc), C.c_void_p(vox.ctypes.data), C.byref(params), C.byref(res)))
        self.result = res
        return res

    def extract_stream(self, desc, source, params):
        """The upload pipeline fed by a producer (include/cuberille_hip.h: cuberille_extract_stream).  source(dst, z0, z1)
        fills the writable numpy array dst ([z1-z0, Ny, Nx], pinned staging memory of the library) with slices [z0, z1)
        -- e.g. mha.open_stream(path), which inflates a compressed MetaImage stretch by stretch.  An exception raised
        by source ends the call (CuberilleError ERR_SOURCE, the exception chained as its cause)."""
        nx, ny, _ = (int(v) for v in desc.dims)
        dtype = np.dtype(PIXEL_DTYPES[int(desc.pixel_type)])
        self._check_view(desc, params, boxed=False)
        raised = []

        def trampoline(_user, dst, z0, z1):
            try:
                n = (z1 - z0) * ny * nx
                buf = (C.c_char * (n * dtype.itemsize)).from_address(dst)
                source(np.frombuffer(buf, dtype=dtype).reshape(z1 - z0, ny, nx), int(z0), int(z1))
                return 0
            except BaseException as e:      # noqa: BLE001 -- must not unwind through the C frame
                raised.append(e)
                return 1

        res = _abi.Result()
        rc = self._lib.cuberille_extract_stream(self._ctx, C.byref(desc), _abi.CHUNK_SOURCE(trampoline), None,
                                                C.byref(params), C.byref(res))
        if rc == _abi.ERR_SOURCE and raised:
            text = self._lib.cuberille_last_error(self._ctx)
            raise _abi.CuberilleError(rc, text.decode("utf-8", "replace") if text else "") from raised[0]
        _abi.check(self._ctx, rc)
        self.result = res
        return res

    def extract_mha(self, path, params):
        """File -> mesh: the MetaImage at `path` is read (and inflated) stretch by stretch straight into the upload
        pipeline; returns (result, stream info with dims / spacing / origin / direction)."""
        from .mha import open_stream
        with open_stream(path) as st:
            desc = make_desc(st.dtype, st.dims, st.spacing, st.origin, st.direction)
            return self.extract_stream(desc, st, params), st

    def extract_device(self, dev_ptr, desc, params, slab=None):
        self._check_view(desc, params)
        res = _abi.Result()
        _abi.check(self._ctx, self._lib.cuberille_extract_device(
            self._ctx, C.byref(desc), C.c_void_p(dev_ptr), C.byref(params),
            C.byref(slab) if slab is not None else None, C.byref(res)))
        self.result = res
        return res

    def count(self, dev_ptr, desc, params, slab=None):
        self._check_view(desc, params)
        npnt, ncell = C.c_uint64(), C.c_uint64()
        _abi.check(self._ctx, self._lib.cuberille_count(
            self._ctx, C.byref(desc), C.c_void_p(dev_ptr), C.byref(params),
            C.byref(slab) if slab is not None else None, C.byref(npnt), C.byref(ncell)))
        return int(npnt.value), int(ncell.value)

    def emit_points(self):
        """Start the offset-free part of the emit (vertex scatter, projection) right after count(); returns at once."""
        _abi.check(self._ctx, self._lib.cuberille_emit_points(self._ctx))

    def emit(self, point_id_offset=0):
        res = _abi.Result()
        _abi.check(self._ctx, self._lib.cuberille_emit(self._ctx, int(point_id_offset), C.byref(res)))
        self.result = res
        return res

    def step_begin(self, dev_ptr, desc, params, slab=None):
        """Count and the offset-free part of the emit, launched back to back without waiting (cuberille_step_begin).
        Returns (device pointer, bytes) of this rank's row, to be all-gathered in rank order."""
        self._check_view(desc, params, boxed=False)
        p, n = C.c_void_p(), C.c_size_t()
        _abi.check(self._ctx, self._lib.cuberille_step_begin(
            self._ctx, C.byref(desc), C.c_void_p(dev_ptr), C.byref(params),
            C.byref(slab) if slab is not None else None, C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def step_classify(self, dev_ptr, desc, params, slab=None):
        """First half of step_begin for the bits-first halo (cuberille_step_classify): thresholds the owned slices and
        returns (device pointer of the buffer's bit volume, words per slice) without waiting."""
        self._check_view(desc, params, boxed=False)
        p, n = C.c_void_p(), C.c_size_t()
        _abi.check(self._ctx, self._lib.cuberille_step_classify(
            self._ctx, C.byref(desc), C.c_void_p(dev_ptr), C.byref(params),
            C.byref(slab) if slab is not None else None, C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def step_count(self, halo_bits_event=None, halo_voxels_event=None):
        """Second half (cuberille_step_count): the count behind halo_bits_event, the walk behind halo_voxels_event (raw
        hipEvent_t handles, e.g. torch.cuda.Event.cuda_event; None: nothing to wait for).  Returns the row like step_begin."""
        p, n = C.c_void_p(), C.c_size_t()
        _abi.check(self._ctx, self._lib.cuberille_step_count(
            self._ctx, C.c_void_p(halo_bits_event or 0), C.c_void_p(halo_voxels_event or 0), C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def step_end(self, dev_rows, n_ranks, rank):
        """The cells with the id offset computed on the device from the gathered rows, then the one wait of the step.
        Returns (result, done): done is False (CUBERILLE_RETRY) when a flag on some rank sends every rank to the
        synchronous calls; the result then only holds the counts."""
        res = _abi.Result()
        rc = self._lib.cuberille_step_end(self._ctx, C.c_void_p(dev_rows), int(n_ranks), int(rank), C.byref(res))
        if rc == _abi.RETRY:
            return res, False
        _abi.check(self._ctx, rc)
        self.result = res
        return res, True

    def slice_counts(self, n_slices):
        """(points, quads) created / emitted by every owned slice of the last count: two uint64 arrays."""
        pts = np.empty(n_slices, dtype=np.uint64)
        quads = np.empty(n_slices, dtype=np.uint64)
        _abi.check(self._ctx, self._lib.cuberille_slice_counts(self._ctx, C.c_void_p(pts.ctypes.data),
                                                                C.c_void_p(quads.ctypes.data), int(n_slices)))
        return pts, quads

    def escaped_count(self):
        """THIN_HALO slabs, after emit_points(): walks that left the buffer (waits for the vertex phase)."""
        n = C.c_uint64()
        _abi.check(self._ctx, self._lib.cuberille_escaped_count(self._ctx, C.byref(n)))
        return _abi.ESCAPED_OVERFLOW if n.value == 2 ** 64 - 1 else int(n.value)

    def reproject_escaped(self, dev_ptr, z_begin, nz):
        """Walk the escaped vertices again in a buffer that holds the full halo (slices [z_begin, z_begin + nz))."""
        _abi.check(self._ctx, self._lib.cuberille_reproject_escaped(self._ctx, C.c_void_p(dev_ptr), int(z_begin), int(nz)))

    # -- results -----------------------------------------------------------------------------
    def download(self, out=None):
        """The last mesh part as numpy arrays.  out: a Mesh of a previous download whose arrays are written again when
        the shapes match -- memory that has been touched before takes the copy at the link's rate, a fresh array is
        bound by its page faults."""
        res = self.result
        npnt, ncell, vpc = int(res.n_points), int(res.n_cells), int(res.verts_per_cell)
        if out is not None and out.points.shape == (npnt, 3) and out.cells.shape == (ncell, vpc) \
                and out.points.dtype == np.float32 and out.cells.dtype == np.uint64 \
                and out.points.flags.c_contiguous and out.cells.flags.c_contiguous:
            pts, cells = out.points, out.cells
        else:
            pts = np.empty((npnt, 3), dtype=np.float32)
            cells = np.empty((ncell, vpc), dtype=np.uint64)
        _abi.check(self._ctx, self._lib.cuberille_mesh_download(
            self._ctx, C.c_void_p(pts.ctypes.data), C.c_void_p(cells.ctypes.data)))
        return Mesh(pts, cells)

    def mesh_host(self):
        """The last mesh part in host memory of the CONTEXT (cuberille_mesh_host): numpy views, valid until the next count
        or extraction on this extractor -- copy what must live longer.  The context keeps the memory across extractions
        (huge pages where the system has them), so this is the fast way to the host for a series of meshes."""
        res = self.result
        npnt, ncell, vpc = int(res.n_points), int(res.n_cells), int(res.verts_per_cell)
        pp, cp = C.c_void_p(), C.c_void_p()
        _abi.check(self._ctx, self._lib.cuberille_mesh_host(self._ctx, C.byref(pp), C.byref(cp)))
        pts = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_float)), shape=(max(npnt * 3, 1),))[:npnt * 3].reshape(npnt, 3)
        cells = np.ctypeslib.as_array(C.cast(cp, C.POINTER(C.c_uint64)), shape=(max(ncell * vpc, 1),))[:ncell * vpc].reshape(ncell, vpc)
        return Mesh(pts, cells)

    def release_host_mesh(self):
        """Give the host memory behind mesh_host() back to the system (views handed out before become invalid)."""
        _abi.check(self._ctx, self._lib.cuberille_release_host_mesh(self._ctx))

    def hold_gradient(self, hold=True):
        """Quirk Q3 of the reference on request (cuberille_hold_gradient; txx:484): like the reference's filter object, this
        extractor keeps the gradient image (and geometry) of its next projecting extraction and walks every later volume
        along it.  hold=False drops the image and returns to the default: each volume's own gradient."""
        _abi.check(self._ctx, self._lib.cuberille_hold_gradient(self._ctx, 1 if hold else 0))

    def set_border(self, width, value=0):
        """Close the surface at the image border without a padded copy (cuberille_set_border): every later whole-volume
        extraction gives the mesh of the image with a ring of `width` (0: off, or 1) voxels of `value` around it -- dims + 2,
        index_start - 1, the same origin, spacing and direction: what itk::ConstantPadImageFilter hands the reference.  The
        value converts to the pixel type like the iso value (an integer past 2^53 reaches the 64-bit integer types whole).
        Slabs, steps, groups, the B-spline interpolator, a held or recursive-Gaussian gradient and the two projection
        variants are refused at the extraction."""
        exact = iso_int_of(value)
        as_int = 0 if exact is None else ((exact + (1 << 63)) % (1 << 64)) - (1 << 63)
        _abi.check(self._ctx, self._lib.cuberille_set_border(self._ctx, int(width), float(value), as_int))
        self._view["border"] = (int(width), exact)

    def set_band(self, lower, upper, inside=1, outside=0):
        """Mesh a label or a value band in place (cuberille_set_band): every later whole-volume extraction gives the mesh of
        B = (lower <= pixel <= upper) ? inside : outside -- what itk::BinaryThresholdImageFilter hands the reference, all four
        values in the pixel type, a NaN pixel outside -- bit for bit, without B: the sweep evaluates the band, the walk maps
        every pixel it loads.  The iso value and all other parameters stay the caller's and apply to B.  The values are checked
        against the pixel type at the extraction (check_band).  Slabs, steps, groups, extract_stream, set_border, set_region,
        the B-spline interpolator, a held or recursive-Gaussian gradient and the two projection variants are refused there."""
        v, vi, _ = _band_arrays((lower, upper, inside, outside))
        _abi.check(self._ctx, self._lib.cuberille_set_band(self._ctx, 1, v, vi))
        self._view["band"] = (lower, upper, inside, outside)

    def clear_band(self):
        """Back to the default: the pixels are thresholded against the iso value themselves."""
        _abi.check(self._ctx, self._lib.cuberille_set_band(self._ctx, 0, None, None))
        self._view["band"] = None

    def set_region(self, start_xyz, size_xyz):
        """Extract a box of a larger volume in place (cuberille_set_region): every later whole-volume extraction still takes
        the description and the pointer of the WHOLE buffer and gives the mesh of the box [start, start + size) -- that of
        the cropped copy with its index kept (region_desc), bit for bit, without the copy: on the device the sweep and the
        walk read the caller's buffer by its pitches, extract_host uploads the box alone.  start is a position in the buffer
        (x, y, z).  Slabs, steps, groups, extract_stream, set_border, the B-spline interpolator, a held or
        recursive-Gaussian gradient and the two projection variants are refused at the extraction."""
        start = (C.c_int64 * 3)(*[int(v) for v in start_xyz])
        size = (C.c_int64 * 3)(*[int(v) for v in size_xyz])
        _abi.check(self._ctx, self._lib.cuberille_set_region(self._ctx, start, size))
        self._view["region"] = None if not any(int(v) for v in size_xyz) else (tuple(int(v) for v in start_xyz), tuple(int(v) for v in size_xyz))

    def clear_region(self):
        """Back to the default: the buffer handed over is the image."""
        _abi.check(self._ctx, self._lib.cuberille_set_region(self._ctx, None, None))
        self._view["region"] = None

    def set_point_normals(self, on=True):
        """Point normals (cuberille_set_point_normals): every later extraction also leaves, for every point, the normalised
        interpolated gradient of the image at the point's final position -- the vector the walk evaluates in every pass
        (txx:451-452), once more where the vertex ended up (or at the lattice start with the projection off).  It points
        towards increasing pixel values: into an object brighter than its surroundings.  A zero gradient gives NaN (quirk
        Q4).  Points, cells and counters are unchanged.  Slabs, steps, groups, a held gradient and the recursive-Gaussian
        gradient are refused at the extraction.  Off (the default) frees the buffer."""
        _abi.check(self._ctx, self._lib.cuberille_set_point_normals(self._ctx, 1 if on else 0))

    def download_normals(self):
        """The normals of the last extraction as a float32 array (n, 3), in point-id order (cuberille_normals_download);
        CuberilleError ERR_STATE when that extraction ran with the setting off."""
        n = int(self.result.n_points) if self.result is not None else 0
        out = np.empty((n, 3), dtype=np.float32)
        _abi.check(self._ctx, self._lib.cuberille_normals_download(self._ctx, C.c_void_p(out.ctypes.data)))
        return out

    def normals_device(self):
        """Device pointer of the normals of the last extraction, 3 floats per point in the library's buffer
        (cuberille_normals_device; it may be None for an empty mesh)."""
        p = C.c_void_p()
        _abi.check(self._ctx, self._lib.cuberille_normals_device(self._ctx, C.byref(p)))
        return p.value

    def set_point_scalars(self, image, outside=float("nan")):
        """Point scalars (cuberille_set_point_scalars): every later extraction also leaves, for every point, the linearly
        interpolated value of a SECOND image at the point's final position -- what a host loop of
        itk::LinearInterpolateImageFunction::Evaluate over the mesh's points gives -- as a double, and `outside` (bit for bit)
        where the point lies outside that image's buffer.  image: a Volume in host memory (the library uploads a copy of its
        own at this call), a (dev_ptr, desc) pair (borrowed: valid and filled until the setting goes off; it may be the volume
        being extracted), or None (off, the default: frees the row and the copy).  Points, cells and counters are unchanged.
        Slabs, steps and groups are refused at the extraction."""
        _set_point_scalars(self._lib, self._ctx, image, outside)

    def download_point_scalars(self):
        """The point scalars of the last extraction as a float64 array of length n_points, in point-id order
        (cuberille_point_scalars_download); CuberilleError ERR_STATE when that extraction ran with the setting off."""
        n = int(self.result.n_points) if self.result is not None else 0
        out = np.empty(n, dtype=np.float64)
        _abi.check(self._ctx, self._lib.cuberille_point_scalars_download(self._ctx, C.c_void_p(out.ctypes.data), out.nbytes))
        return out

    def point_scalars_device(self):
        """Device pointer of the point scalars of the last extraction, one double per point in the library's buffer
        (cuberille_point_scalars_device; None for an empty mesh)."""
        p = C.c_void_p()
        _abi.check(self._ctx, self._lib.cuberille_point_scalars_device(self._ctx, C.byref(p)))
        return p.value

    def set_cell_pixels(self, on=True):
        """Cell pixels (cuberille_set_cell_pixels): every later extraction also leaves, for every cell, the pixel of the
        inside voxel of the cell's quad, in the volume's own dtype -- the value the reference's commented-out SetCellData
        (txx:314, 321, 330) would carry.  Both triangles of a quad carry the quad's pixel.  With a band it is the caller's raw
        pixel (which label), with a border the padded image's, with a region the box's.  Points, cells and counters are
        unchanged.  Slabs, steps and groups are refused at the extraction.  Off (the default) frees the buffer."""
        _abi.check(self._ctx, self._lib.cuberille_set_cell_pixels(self._ctx, 1 if on else 0))

    def cell_pixels_device(self):
        """(device pointer, CUBERILLE_PIX_* type) of the cell pixels of the last extraction, one value per cell in the
        library's buffer (cuberille_cell_pixels_device; the pointer is None for an empty mesh)."""
        p, t = C.c_void_p(), C.c_int(-1)
        _abi.check(self._ctx, self._lib.cuberille_cell_pixels_device(self._ctx, C.byref(p), C.byref(t)))
        return p.value, int(t.value)

    def download_cell_pixels(self):
        """The cell pixels of the last extraction as a numpy array of the volume's dtype and length n_cells, in cell order
        (cuberille_cell_pixels_download); CuberilleError ERR_STATE when that extraction ran with the setting off."""
        _, t = self.cell_pixels_device()
        dtype = np.dtype(PIXEL_DTYPES[t])
        n = int(self.result.n_cells) if self.result is not None else 0
        out = np.empty(n, dtype=dtype)
        _abi.check(self._ctx, self._lib.cuberille_cell_pixels_download(self._ctx, C.c_void_p(out.ctypes.data), out.nbytes))
        return out

    def set_components(self, on=True):
        """Surface components (cuberille_set_components): every later extraction also labels the connected surfaces of its
        mesh on the device -- two points are joined when one cell holds both, components are numbered in the order of their
        smallest point index.  Points, cells and counters are unchanged.  Slabs, steps and groups are refused at the
        extraction.  Off (the default) frees the rows."""
        _abi.check(self._ctx, self._lib.cuberille_set_components(self._ctx, 1 if on else 0))

    def n_components(self):
        """K, the number of components of the last extraction (cuberille_components_info); CuberilleError ERR_STATE when that
        extraction ran with the setting off."""
        k = C.c_uint64()
        _abi.check(self._ctx, self._lib.cuberille_components_info(self._ctx, C.byref(k)))
        return int(k.value)

    def components_device(self):
        """Device pointers (point_component, cell_component, component_cells) of the last extraction, in the library's
        buffers (cuberille_components_device; None each for an empty mesh)."""
        p, q, r = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _abi.check(self._ctx, self._lib.cuberille_components_device(self._ctx, C.byref(p), C.byref(q), C.byref(r)))
        return p.value, q.value, r.value

    def download_components(self):
        """(point_component uint32[n_points], cell_component uint32[n_cells], component_cells uint64[K]) of the last
        extraction as numpy arrays (cuberille_components_download)."""
        k = self.n_components()
        n_points = int(self.result.n_points) if self.result is not None else 0
        n_cells = int(self.result.n_cells) if self.result is not None else 0
        pc, cc, counts = np.empty(n_points, np.uint32), np.empty(n_cells, np.uint32), np.empty(k, np.uint64)
        _abi.check(self._ctx, self._lib.cuberille_components_download(
            self._ctx, C.c_void_p(pc.ctypes.data), C.c_void_p(cc.ctypes.data), C.c_void_p(counts.ctypes.data), k))
        return pc, cc, counts

    _KEEP_RULES = {"largest": _abi.KEEP_LARGEST, "min_cells": _abi.KEEP_MIN_CELLS, "mask": _abi.KEEP_MASK}

    def keep_components(self, rule, n=0, mask=None):
        """Compact the last mesh by component on the device (cuberille_keep_components): rule "largest" (the one component
        with the most cells, a tie to the smaller number), "min_cells" (every component of at least n cells) or "mask"
        (component k is kept when mask[k] is non-zero: K entries), or the _abi.KEEP_* constants.  The mesh must have come
        with components (set_components).  download(), mesh_host(), download_normals(), download_cell_pixels(),
        download_components(), n_components() and write_vtk() then speak of the kept mesh; self.result becomes a copy with
        the new n_points and n_cells, its counters and times those of the extraction.  Returns
        (n_points, n_cells, n_components, ms)."""
        rule = self._KEEP_RULES.get(rule, rule) if isinstance(rule, str) else int(rule)
        if isinstance(rule, str):
            raise _abi.CuberilleError(_abi.ERR_ARGUMENT, "keep_components: unknown rule %r" % (rule,))
        m, ptr, length = None, None, 0
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            ptr, length = C.c_void_p(m.ctypes.data), int(m.size)
        npnt, ncell, k, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
        _abi.check(self._ctx, self._lib.cuberille_keep_components(self._ctx, rule, int(n), ptr, length, C.byref(npnt), C.byref(ncell),
                                                                  C.byref(k), C.byref(ms)))
        if self.result is not None:
            res = type(self.result).from_buffer_copy(self.result)      # (the caller's result of the extraction stays as it was)
            res.n_points, res.n_cells = npnt.value, ncell.value
            self.result = res
        return int(npnt.value), int(ncell.value), int(k.value), float(ms.value)

    def device_bytes(self):
        """Bytes of device memory the context's workspace holds at this moment (cuberille_debug_device_bytes)."""
        n = C.c_size_t()
        _abi.check(self._ctx, self._lib.cuberille_debug_device_bytes(self._ctx, C.byref(n)))
        return int(n.value)

    def set_interpolator(self, kind, spline_order=3, coordinate_bits=32, coefficient_bits=32):
        """The value interpolator of the walk for the later extractions (cuberille_set_interpolator): _abi.INTERP_LINEAR
        (the default) or _abi.INTERP_BSPLINE -- itk::BSplineInterpolateImageFunction of spline_order 3, <float, float>
        (bits 32, 32) or <double, double> (64, 64), its coefficient image computed on the device."""
        _abi.check(self._ctx, self._lib.cuberille_set_interpolator(self._ctx, int(kind), int(spline_order), int(coordinate_bits),
                                                                   int(coefficient_bits)))

    def bspline_coefficients(self, dims_xyz=None, bits=None):
        """The coefficient image of the last B-spline extraction as an array (nz, ny, nx) of float32 / float64, sized from
        the context's own record of it (cuberille_bspline_coefficients_info).  dims_xyz / bits, when given, must match it."""
        dims = (C.c_int64 * 3)()
        have = C.c_int()
        if not self._lib.cuberille_bspline_coefficients_info(self._ctx, dims, C.byref(have)):
            raise _abi.CuberilleError(_abi.ERR_STATE, "no B-spline extraction on this context has projected a vertex")
        nx, ny, nz = (int(v) for v in dims)
        if dims_xyz is not None and tuple(int(v) for v in dims_xyz) != (nx, ny, nz):
            raise ValueError("the coefficient image held is %dx%dx%d, not %s" % (nx, ny, nz, tuple(dims_xyz)))
        if bits is not None and int(bits) != have.value:
            raise ValueError("the coefficient image held is %d bits wide, not %d" % (have.value, bits))
        out = np.empty((nz, ny, nx), dtype=np.float64 if have.value == 64 else np.float32)
        _abi.check(self._ctx, self._lib.cuberille_bspline_coefficients(self._ctx, C.c_void_p(out.ctypes.data), out.nbytes))
        return out

    @property
    def gradient_held(self):
        """None, or the (nz, ny, nx) of the volume whose gradient image the extractor holds."""
        dims = (C.c_int64 * 3)()
        if not self._lib.cuberille_gradient_held(self._ctx, dims):
            return None
        return (int(dims[2]), int(dims[1]), int(dims[0]))

    def write_vtk(self, path, threads=0):
        """Download the last whole-volume mesh and write it as legacy-ASCII VTK POLYDATA."""
        _abi.check(self._ctx, self._lib.cuberille_mesh_write_vtk(self._ctx, os.fsencode(path), int(threads)))

    def device_pointers(self):
        p, c = C.c_void_p(), C.c_void_p()
        _abi.check(self._ctx, self._lib.cuberille_mesh_device(self._ctx, C.byref(p), C.byref(c)))
        return p.value, c.value

    def debug_bits(self, dims_xyz):
        nx, ny, nz = dims_xyz
        W = (nx + 63) // 64
        words = np.empty((nz, ny, W), dtype=np.uint64)
        _abi.check(self._ctx, self._lib.cuberille_debug_bits(self._ctx, C.c_void_p(words.ctypes.data), words.size))
        return words

    def slice_occupancy(self, nz):
        occ = np.empty(nz, dtype=np.uint32)
        _abi.check(self._ctx, self._lib.cuberille_slice_occupancy(self._ctx, C.c_void_p(occ.ctypes.data), nz))
        return occ != 0

    def slab_info(self):
        """After count() on a slab: SlabInfo(alias_below, lowest, highest, second_highest, alias_z) -- the fields of
        cuberille_slab_status (global slices, -1 = none)."""
        st = _abi.SlabStatus()
        _abi.check(self._ctx, self._lib.cuberille_slab_info(self._ctx, C.byref(st)))
        return SlabInfo(bool(st.alias_source_below_buffer), int(st.lowest_occupied_z), int(st.highest_occupied_z),
                        int(st.second_highest_occupied_z), int(st.alias_z))

    # -- quirk Q1 across a slab boundary (include/cuberille_hip.h) ------------------------------------------------
    def slice_bits_device(self, z_global):
        """(device pointer, n_words) of the inside bits of one buffer slice."""
        p, n = C.c_void_p(), C.c_size_t()
        _abi.check(self._ctx, self._lib.cuberille_slice_bits_device(self._ctx, int(z_global), C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def recount(self, dev_source_bits):
        npnt, ncell = C.c_uint64(), C.c_uint64()
        _abi.check(self._ctx, self._lib.cuberille_recount(self._ctx, C.c_void_p(dev_source_bits), C.byref(npnt), C.byref(ncell)))
        return int(npnt.value), int(ncell.value)

    def alias_plane_device(self, z_global, dev_ids, dev_points):
        _abi.check(self._ctx, self._lib.cuberille_alias_plane_device(self._ctx, int(z_global), C.c_void_p(dev_ids),
                                                                     C.c_void_p(dev_points)))

    def set_alias_plane(self, dev_ids, dev_points):
        _abi.check(self._ctx, self._lib.cuberille_set_alias_plane(self._ctx, C.c_void_p(dev_ids), C.c_void_p(dev_points)))

    def debug_option(self, name, value):
        """Development switch of this context (cuberille_debug_set_option); "defaults" resets them all."""
        _abi.check(self._ctx, self._lib.cuberille_debug_set_option(self._ctx, name.encode(), int(value)))


def required_halo(desc, params):
    """Slices a slab buffer must hold (below, above) its owned range for these parameters (needs no GPU)."""
    lo, hi = C.c_int64(), C.c_int64()
    rc = _abi.lib().cuberille_required_halo(C.byref(desc), C.byref(params), C.byref(lo), C.byref(hi))
    if rc != _abi.OK:
        raise _abi.CuberilleError(rc, "cuberille_required_halo: bad image description or parameters")
    return int(lo.value), int(hi.value)


def minimum_halo(desc, params):
    """The least a THIN_HALO slab must hold (below, above) its owned range (needs no GPU)."""
    lo, hi = C.c_int64(), C.c_int64()
    rc = _abi.lib().cuberille_minimum_halo(C.byref(desc), C.byref(params), C.byref(lo), C.byref(hi))
    if rc != _abi.OK:
        raise _abi.CuberilleError(rc, "cuberille_minimum_halo: bad image description or parameters")
    return int(lo.value), int(hi.value)


def group_plan(desc, params, n):
    """The cuts a group of n contexts makes of this image for these parameters (cuberille_group_plan, needs no GPU):
    [(own_z0, own_z1, buf_z0, buf_z1)] for the min(n, Nz) slabs that take part."""
    n = int(n)
    bounds = (C.c_int64 * (4 * max(n, 1)))()
    used = C.c_int()
    rc = _abi.lib().cuberille_group_plan(C.byref(desc), C.byref(params), n, bounds, C.byref(used))
    if rc != _abi.OK:
        raise _abi.CuberilleError(rc, "cuberille_group_plan: %d members, or these parameters, are not offered" % n)
    return [tuple(int(v) for v in bounds[4 * i:4 * i + 4]) for i in range(used.value)]


class ExtractorGroup:
    """Several contexts driven together (include/cuberille_hip.h: cuberille_group): a host-resident volume is cut into
    z-slabs of equal thickness, each uploaded with its full halo straight from host memory to its member's device, and
    one mesh comes back -- the same ids, cell order and bits as Extractor.extract_host of the whole volume.  devices: one
    device id per member; ids may repeat (several contexts on one GPU)."""

    def __init__(self, devices):
        self._lib = _abi.lib()
        self._g = C.c_void_p()
        ids = [int(d) for d in devices]
        arr = (C.c_int * max(len(ids), 1))(*ids)
        rc = self._lib.cuberille_group_create(C.byref(self._g), arr, len(ids))
        if rc != _abi.OK:
            text = self._lib.cuberille_group_last_error(None)
            self._g = C.c_void_p()
            raise _abi.CuberilleError(rc, text.decode() if text else "")
        self.devices = ids
        self.result = None

    def close(self):
        if getattr(self, "_g", None) is not None and self._g:
            self._lib.cuberille_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def plan(self, desc, params):
        """[(own_z0, own_z1, buf_z0, buf_z1)] per slab this group would cut for desc (needs no GPU)."""
        return group_plan(desc, params, len(self.devices))

    def warm_up(self, desc=None, params=None):
        """cuberille_group_warm_up: every member loads its code objects and, with an image description, reserves the
        workspace of its slab."""
        _abi.check_group(self._g, self._lib.cuberille_group_warm_up(self._g, C.byref(desc) if desc is not None else None,
                                                                    C.byref(params) if params is not None else None))

    def context(self, i):
        """The raw cuberille_ctx pointer of member i (for cuberille_debug_set_option and the like)."""
        p = self._lib.cuberille_group_context(self._g, int(i))
        if not p:
            raise IndexError("member %d of a group of %d" % (i, len(self.devices)))
        return C.c_void_p(p)

    def debug_option(self, i, name, value):
        """Development switch of member i (cuberille_debug_set_option)."""
        ctx = self.context(i)
        _abi.check(ctx, self._lib.cuberille_debug_set_option(ctx, name.encode(), int(value)))

    def _on_every_member(self, setter, *args):
        for i in range(len(self.devices)):
            ctx = self.context(i)
            _abi.check(ctx, setter(ctx, *args))

    def set_border(self, width, value=0):
        """An implied border (Extractor.set_border) on every member: the group's extraction then raises the library's
        refusal -- the ring would have to reach across the slabs."""
        self._on_every_member(self._lib.cuberille_set_border, int(width), float(value), 0)

    def set_band(self, lower, upper, inside=1, outside=0):
        """A band (Extractor.set_band) on every member: the group's extraction then raises the library's refusal -- the binary
        image belongs to one context's whole volume."""
        v, vi, _ = _band_arrays((lower, upper, inside, outside))
        self._on_every_member(self._lib.cuberille_set_band, 1, v, vi)

    def set_region(self, start_xyz, size_xyz):
        """A region (Extractor.set_region) on every member: the group's extraction then raises the library's refusal -- a
        box belongs to one context's whole volume."""
        start = (C.c_int64 * 3)(*[int(v) for v in start_xyz])
        size = (C.c_int64 * 3)(*[int(v) for v in size_xyz])
        self._on_every_member(self._lib.cuberille_set_region, start, size)

    def set_point_normals(self, on=True):
        """Point normals (Extractor.set_point_normals) on every member: the group's extraction then raises the library's
        refusal -- they belong to one context's whole volume."""
        self._on_every_member(self._lib.cuberille_set_point_normals, 1 if on else 0)

    def set_cell_pixels(self, on=True):
        """Cell pixels (Extractor.set_cell_pixels) on every member: the group's extraction then raises the library's
        refusal -- they belong to one context's whole volume."""
        self._on_every_member(self._lib.cuberille_set_cell_pixels, 1 if on else 0)

    def set_point_scalars(self, image, outside=float("nan")):
        """Point scalars (Extractor.set_point_scalars) on every member: the group's extraction then raises the library's
        refusal -- they belong to one context's whole volume."""
        for i in range(len(self.devices)):
            _set_point_scalars(self._lib, self.context(i), image, outside)

    def set_components(self, on=True):
        """Components (Extractor.set_components) on every member: the group's extraction then raises the library's
        refusal -- a component does not stop at a slab's face."""
        self._on_every_member(self._lib.cuberille_set_components, 1 if on else 0)

    def debug_fail_alloc(self, slab, n):
        """Failure drill: the n-th device allocation of slab `slab`'s upload and count in the next extraction fails
        (slab -1: every slab's; n < 0: off)."""
        _abi.check_group(self._g, self._lib.cuberille_group_debug_fail_alloc(self._g, int(slab), int(n)))

    def extract_host(self, vol, params):
        """vol: mha.Volume in host memory.  Upload + extract on every member; the summed result (device times: the
        largest of the slabs')."""
        vox = np.ascontiguousarray(vol.voxels)
        desc = make_desc(vox.dtype, vol.dims, vol.spacing, vol.origin, vol.direction, getattr(vol, "index_start", (0, 0, 0)))
        check_iso(int(desc.pixel_type), params)
        res = _abi.Result()
        _abi.check_group(self._g, self._lib.cuberille_group_extract_host(
            self._g, C.byref(desc), C.c_void_p(vox.ctypes.data), C.byref(params), C.byref(res)))
        self.result = res
        return res

    def slab_result(self, i):
        """Slab i's own result of the last extraction."""
        res = _abi.Result()
        _abi.check_group(self._g, self._lib.cuberille_group_slab_result(self._g, int(i), C.byref(res)))
        return res

    def download(self):
        """The assembled mesh of the last extraction, copied out of the group's host memory."""
        res = self.result
        npnt, ncell, vpc = int(res.n_points), int(res.n_cells), int(res.verts_per_cell)
        pp, cp = C.c_void_p(), C.c_void_p()
        _abi.check_group(self._g, self._lib.cuberille_group_mesh_host(self._g, C.byref(pp), C.byref(cp)))
        pts = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_float)), shape=(max(npnt * 3, 1),))[:npnt * 3]
        cells = np.ctypeslib.as_array(C.cast(cp, C.POINTER(C.c_uint64)), shape=(max(ncell * vpc, 1),))[:ncell * vpc]
        return Mesh(pts.reshape(npnt, 3).copy(), cells.reshape(ncell, vpc).copy())

    def release_host_mesh(self):
        _abi.check_group(self._g, self._lib.cuberille_group_release_host_mesh(self._g))

    def write_vtk(self, path, threads=0):
        """The assembled mesh as legacy-ASCII VTK polydata (cuberille_group_mesh_write_vtk)."""
        _abi.check_group(self._g, self._lib.cuberille_group_mesh_write_vtk(self._g, os.fsencode(path), int(threads)))


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def _pixel_max(dt):
    dt = np.dtype(dt)
    return float(np.iinfo(dt).max) if dt.kind in "iu" else float(np.finfo(dt).max)


class CuberilleImageToMeshFilter:
    """Python mirror of itk::CuberilleImageToMeshFilter (h:110-339).

    Input: mha.Volume (host memory, like the itk::Image the reference driver hands
    over).  Output: Mesh with the reference's vertex ids, cell order and coordinates.
    """

    # Off unless InsideBandOn: the one default kept at class level, since Update() reads it on every call and a filter made
    # without __init__ (tests/test_region.py::test_python_filter_index_arithmetic) has only what Update() read before the band
    _band_on = False

    # The view settings that several devices do not offer: (attribute, its "off", the setting by name, why)
    _normals = False       # SetGeneratePointNormals: off (class level for the same reason)
    _cell_pixels_on = False   # SetSavePixelAsCellData: off (likewise)
    _components_on = False    # SetGenerateComponents: off (likewise)
    _keep_largest = False     # SetKeepLargestComponent: off (likewise)
    _min_component_cells = 0  # SetMinimumComponentCells: none (likewise)
    _scalar_image = None      # SetPointScalarImage: none (likewise)

    _NOT_IN_A_GROUP = (
        ("_pad_border", False, "an implied border (SetPadBorder / cuberille_set_border)", "the ring would have to reach across slabs"),
        ("_region", None, "a region (SetExtractionRegion / cuberille_set_region)", "a box belongs to one context's whole volume"),
        ("_band_on", False, "a band (InsideBandOn / cuberille_set_band)", "the binary image belongs to one context's whole volume"),
        ("_normals", False, "point normals (SetGeneratePointNormals / cuberille_set_point_normals)", "they belong to one context's whole volume"),
        ("_cell_pixels_on", False, "cell pixels (SetSavePixelAsCellData / cuberille_set_cell_pixels)", "they belong to one context's whole volume"),
        ("_components_on", False, "components (SetGenerateComponents / cuberille_set_components)", "a component does not stop at a slab's face"),
        ("_keep_largest", False, "the largest component (SetKeepLargestComponent / cuberille_keep_components)", "a component does not stop at a slab's face"),
        ("_scalar_image", None, "point scalars (SetPointScalarImage / cuberille_set_point_scalars)", "they belong to one context's whole volume"),
        ("_min_component_cells", 0, "a minimum of cells per component (SetMinimumComponentCells / cuberille_keep_components)", "a component does not stop at a slab's face"))

    def __init__(self, device=0, devices=None):
        self._device = device
        self._devices = [int(d) for d in devices] if devices else []
        self._group = None
        self.last_number_of_slabs = 0
        self._extractor = None
        self._input = None
        self._output = None
        self._dtype = np.dtype(np.uint8)
        # txx:33-40
        self._iso = 1
        self._triangles = True
        self._project = True
        self._threshold = self._threshold_asked = 0.5
        self._step = -1.0
        self._relax = 0.95
        self._max_steps = 50
        self._q1 = True
        self._variant = PROJECT_DEFAULT           # h:22-23: both alternative branches are compiled out
        self._gradient = GRADIENT_CENTRAL         # h:21: and so is the recursive-Gaussian gradient
        self._stale_gradient = False
        self._bspline = None                      # (coordinate bits, coefficient bits) of SetBSplineInterpolator, or None
        self._pad_border = False                  # SetPadBorder: off, like the reference
        self._border_pad_value = 0                # SetBorderPadValue: NumericTraits<InputPixelType>::Zero
        self._region = None                       # SetExtractionRegion: (index_xyz, size_xyz) in ITK index space, or None
        self._band = (0, 0)                       # SetInsideBand: lower, upper
        self._band_values = (1, 0)                # SetBandValues: NumericTraits<InputPixelType>::One / Zero
        self._normals = False                     # SetGeneratePointNormals: off
        self._point_normals = None                # GetPointNormals(): (n, 3) float32 of the last Update(), or None
        self._cell_pixels_on = False              # SetSavePixelAsCellData: off
        self._cell_pixels = None                  # GetCellPixels(): one pixel per cell of the last Update(), or None
        self._components_on = False               # SetGenerateComponents: off
        self._components = None                   # (point_component, cell_component, component_cells) of the last Update(), or None
        self._keep_largest = False                # SetKeepLargestComponent: off
        self._min_component_cells = 0             # SetMinimumComponentCells: none
        self._scalar_image = None                 # SetPointScalarImage: the second image (a Volume), or None
        self._scalar_outside = float("nan")       # SetPointScalarOutsideValue
        self._scalar_uploaded = False             # ... the extractor holds its copy of that image
        self._point_scalars = None                # GetPointScalars(): float64 per point of the last Update(), or None
        self.last_result = None
        # like the C++ drop-in: the GPU context and the code objects are set up when the filter is made, not inside the
        # first Update() (the reference's driver times one cold Update(), test:158-160); silent without a device --
        # Update() tries again and raises
        self._acquire(False)

    def _acquire(self, must):
        if self._extractor is None:
            try:
                self._extractor = Extractor(self._device)
                self._extractor.warm_up()
            except (_abi.CuberilleError, ImportError, OSError):
                self._extractor = None
                if must:
                    raise
        return self._extractor is not None

    # h:184 / txx:53-56
    def SetInput(self, image):
        if not isinstance(image, Volume):
            raise TypeError("SetInput expects an mha.Volume")
        self._input = image
        self._dtype = image.voxels.dtype
        self._threshold = _clamp(self._threshold_asked, 0.0, _pixel_max(self._dtype))
        if self._acquire(False) and self._dtype in PIXEL_CODES:
            self._extractor.warm_up(make_desc(self._dtype, image.dims, image.spacing, image.origin, image.direction, image.index_start))

    def SetDevices(self, devices):
        """Not in the reference (like the C++ drop-in's SetDevices): more than one device id -- ids may repeat -- makes
        Update() cut the volume into z-slabs, one per member of an ExtractorGroup, where the parameters are ones a slab
        takes; otherwise (an empty list, the default, or the B-spline interpolator, a reproduced stale gradient or the
        recursive-Gaussian gradient) it runs on `device` alone."""
        self._devices = [int(d) for d in devices] if devices else []
        if self._group is not None and self._group.devices != self._devices:
            self._group.close()
            self._group = None

    def GetDevices(self):
        return list(self._devices)

    def GetLastNumberOfSlabs(self):
        """Slabs the last Update() was cut into: 1 on the single context."""
        return self.last_number_of_slabs

    # h:180-181
    def SetIsoSurfaceValue(self, v):
        self._iso = v

    def GetIsoSurfaceValue(self):
        return self._iso

    # h:193-195
    def SetGenerateTriangleFaces(self, b):
        self._triangles = bool(b)

    def GetGenerateTriangleFaces(self):
        return self._triangles

    def GenerateTriangleFacesOn(self):
        self._triangles = True

    def GenerateTriangleFacesOff(self):
        self._triangles = False

    # h:199-201
    def SetProjectVerticesToIsoSurface(self, b):
        self._project = bool(b)

    def GetProjectVerticesToIsoSurface(self):
        return self._project

    def ProjectVerticesToIsoSurfaceOn(self):
        self._project = True

    def ProjectVerticesToIsoSurfaceOff(self):
        self._project = False

    # h:209-210 clamp [0, max pixel].  The reference knows the pixel type at compile time; here it is known once
    # an input is set, so the upper clamp is (re)applied against the input's type by SetInput and Update
    def SetProjectVertexSurfaceDistanceThreshold(self, v):
        self._threshold_asked = float(v)
        self._threshold = _clamp(float(v), 0.0, _pixel_max(self._dtype) if self._input is not None else float("inf"))

    def GetProjectVertexSurfaceDistanceThreshold(self):
        return self._threshold

    # h:215-216 clamp [0, 100000]
    def SetProjectVertexStepLength(self, v):
        self._step = _clamp(float(v), 0.0, 100000.0)

    def GetProjectVertexStepLength(self):
        return self._step

    # h:222-223 clamp [0, 1]
    def SetProjectVertexStepLengthRelaxationFactor(self, v):
        self._relax = _clamp(float(v), 0.0, 1.0)

    def GetProjectVertexStepLengthRelaxationFactor(self):
        return self._relax

    # h:227-228
    def SetProjectVertexMaximumNumberOfSteps(self, n):
        self._max_steps = int(n)

    def GetProjectVertexMaximumNumberOfSteps(self):
        return self._max_steps

    def SetEmulateEmptySliceAliasing(self, b):
        """Not in the reference: switches the reproduction of its quirk Q1."""
        self._q1 = bool(b)

    def SetProjectionVariant(self, variant):
        """Not in the reference's API: stands for building it with USE_ADVANCED_PROJECTION (1) or
        USE_LINESEARCH_PROJECTION (2) set (h:22-23); 0 is what it ships."""
        if variant not in (PROJECT_DEFAULT, PROJECT_ADVANCED, PROJECT_LINESEARCH):
            raise ValueError("projection variant must be 0, 1 or 2")
        self._variant = int(variant)

    def SetGradientVariant(self, gradient):
        """Not in the reference's API: stands for building it with USE_GRADIENT_RECURSIVE_GAUSSIAN set (h:21)."""
        if gradient not in (GRADIENT_CENTRAL, GRADIENT_RECURSIVE_GAUSSIAN):
            raise ValueError("gradient variant must be 0 or 1")
        self._gradient = int(gradient)

    def SetReproduceStaleGradient(self, b):
        """Not in the reference -- its behaviour, on request (like the C++ drop-in's switch of the same name): the reference's
        gradient interpolator is created once per filter object (txx:484), so every Update() after the first projecting
        one walks along the FIRST input's gradient.  Default off: each input's own gradient."""
        self._stale_gradient = bool(b)

    def GetReproduceStaleGradient(self):
        return self._stale_gradient

    def SetBSplineInterpolator(self, order=3, coordinate=np.float32, coefficient=np.float32):
        """Stands for SetInterpolator(itk::BSplineInterpolateImageFunction<TImage, coordinate, coefficient>) with
        SetSplineOrder(order) -- the reference driver's USE_BSPLINE_INTERPOLATOR configuration -- walked on the device
        (cuberille_set_interpolator).  coordinate / coefficient: float32 or float64 (or 32 / 64), the same for both; order 3.
        Update() then raises on anything the library refuses (a projection variant, the recursive-Gaussian gradient, a
        reproduced stale gradient)."""
        def bits(t):
            return int(t) if isinstance(t, int) else np.dtype(t).itemsize * 8
        cb, kb = bits(coordinate), bits(coefficient)
        if int(order) != 3 or cb != kb or cb not in (32, 64):
            raise ValueError("the device B-spline walk implements order 3 with float32/float32 or float64/float64")
        self._bspline = (cb, kb)

    def SetPadBorder(self, b):
        """Not in the reference -- what its class comment (h:54-57) tells the caller to do by hand: treat the input as if
        itk::ConstantPadImageFilter had padded it by one pixel of GetBorderPadValue() on every side, so that a surface that
        meets the image border is closed there.  No padded copy is made (cuberille_set_border).  Default off."""
        self._pad_border = bool(b)

    def GetPadBorder(self):
        return self._pad_border

    def PadBorderOn(self):
        self.SetPadBorder(True)

    def PadBorderOff(self):
        self.SetPadBorder(False)

    def SetBorderPadValue(self, v):
        """The constant of the implied border, an InputPixelType (default 0, ConstantPadImageFilter's; signed CT data wants
        its minimum)."""
        self._border_pad_value = v

    def GetBorderPadValue(self):
        return self._border_pad_value

    def SetExtractionRegion(self, index_xyz, size_xyz):
        """Not in the reference -- what a caller does there with itk::ExtractImageFilter first: mesh the box of the input that
        starts at ITK index `index_xyz` and has `size_xyz` voxels, as if that filter's output (its index kept) were the
        input.  No cropped copy is made; Update() uploads the box alone (cuberille_set_region).  The box must lie inside the
        input's buffered region: Update() raises the library's message otherwise."""
        self._region = (tuple(int(v) for v in index_xyz), tuple(int(v) for v in size_xyz))

    def ClearExtractionRegion(self):
        self._region = None

    def GetExtractionRegion(self):
        """(index_xyz, size_xyz), or None."""
        return self._region

    def _buffer_region(self, vol):
        """The region as the library takes it: a position in the buffer = ITK index - start index of the input."""
        if self._region is None:
            return None
        s = getattr(vol, "index_start", (0, 0, 0))
        return tuple(int(i) - int(b) for i, b in zip(self._region[0], s)), self._region[1]

    def SetInsideBand(self, lower, upper):
        """Not in the reference -- what a caller does there with itk::BinaryThresholdImageFilter first: with InsideBandOn(),
        mesh the binary image (lower <= pixel <= upper) ? inside : outside as if that filter's output were the input; the iso
        value applies to it.  No thresholded copy is made (cuberille_set_band)."""
        self._band = (lower, upper)

    def SetBandValues(self, inside, outside):
        self._band_values = (inside, outside)

    def InsideBandOn(self):
        self._band_on = True

    def InsideBandOff(self):
        self._band_on = False

    def GetInsideBand(self):
        return self._band_on

    def SetGeneratePointNormals(self, b):
        """Not in the reference -- the vector its walk evaluates in every pass and throws away (txx:451-452): with the switch
        on, Update() also fills GetPointNormals() with the normalised interpolated gradient at every point's final position
        (cuberille_set_point_normals).  It points towards increasing pixel values.  Default off."""
        self._normals = bool(b)

    def GetGeneratePointNormals(self):
        return self._normals

    def GeneratePointNormalsOn(self):
        self.SetGeneratePointNormals(True)

    def GeneratePointNormalsOff(self):
        self.SetGeneratePointNormals(False)

    def GetPointNormals(self):
        """(n, 3) float32 in point-id order, filled by the last Update() with the switch on; None with it off."""
        return self._point_normals

    def SetPointScalarImage(self, volume):
        """Not in the reference -- what a caller does with the mesh afterwards: a second image (a Volume of any pixel type,
        size and geometry) is linearly interpolated at every point's final position, as a host loop of
        itk::LinearInterpolateImageFunction::Evaluate over the mesh's points would (cuberille_set_point_scalars), and Update()
        fills GetPointScalars().  None turns it off (the default).  The image is uploaded once per call of this method: a
        caller who changes its pixels calls it again."""
        self._scalar_image = volume
        self._scalar_uploaded = False

    def SetPointScalarOutsideValue(self, v):
        """The value of a point outside the second image's buffer (default NaN), kept bit for bit."""
        self._scalar_outside = float(v)
        self._scalar_uploaded = False

    def GetPointScalars(self):
        """float64 per point id, filled by the last Update() with a second image set; None without one."""
        return self._point_scalars

    def SetSavePixelAsCellData(self, b):
        """The switch of the filter's maintained successor; the reference reserves the place with a commented-out
        mesh->SetCellData( id, ... ) behind every cell (txx:314, 321, 330).  On: Update() also fills GetCellPixels() with
        the pixel of each cell's inside voxel (cuberille_set_cell_pixels).  Default off."""
        self._cell_pixels_on = bool(b)

    def GetSavePixelAsCellData(self):
        return self._cell_pixels_on

    def SavePixelAsCellDataOn(self):
        self.SetSavePixelAsCellData(True)

    def SavePixelAsCellDataOff(self):
        self.SetSavePixelAsCellData(False)

    def GetCellPixels(self):
        """One value of the input's dtype per cell id, filled by the last Update() with the switch on; None with it off."""
        return self._cell_pixels

    def SetGenerateComponents(self, b):
        """Not in the reference.  On: Update() also labels the connected surfaces of the mesh on the device
        (cuberille_set_components) and fills GetPointComponents() / GetCellComponents() / GetComponentCellCounts() /
        GetNumberOfComponents().  Default off."""
        self._components_on = bool(b)

    def GetGenerateComponents(self):
        return self._components_on

    def GenerateComponentsOn(self):
        self.SetGenerateComponents(True)

    def GenerateComponentsOff(self):
        self.SetGenerateComponents(False)

    def GetPointComponents(self):
        """uint32 per point id, filled by the last Update() with the switch on; None with it off."""
        return None if self._components is None else self._components[0]

    def GetCellComponents(self):
        """uint32 per cell id: the component of the cell's first point; None with the switch off."""
        return None if self._components is None else self._components[1]

    def GetComponentCellCounts(self):
        """uint64 per component: its cells; None with the switch off."""
        return None if self._components is None else self._components[2]

    def GetNumberOfComponents(self):
        """K of the last Update() with the switch on; 0 with it off."""
        return 0 if self._components is None else int(self._components[2].shape[0])

    def SetKeepLargestComponent(self, b):
        """Not in the reference.  On: Update() keeps the one connected surface with the most cells and drops the rest, on the
        device behind the extraction (cuberille_keep_components, LARGEST; a tie goes to the component with the smaller first
        point).  Turns the components on for that extraction by itself; the output, the normals, the cell pixels and the
        component getters describe the kept mesh.  Default off."""
        self._keep_largest = bool(b)

    def GetKeepLargestComponent(self):
        return self._keep_largest

    def KeepLargestComponentOn(self):
        self.SetKeepLargestComponent(True)

    def KeepLargestComponentOff(self):
        self.SetKeepLargestComponent(False)

    def SetMinimumComponentCells(self, n):
        """Not in the reference.  n > 0: Update() drops every connected surface of fewer than n cells (cuberille_keep_components,
        MIN_CELLS; with triangles a quad is two cells), behind the largest-component selection where both are set.  Turns the
        components on for that extraction by itself.  Default 0: nothing is dropped."""
        if int(n) < 0:
            raise ValueError("SetMinimumComponentCells: a count of cells, got %r" % (n,))
        self._min_component_cells = int(n)

    def GetMinimumComponentCells(self):
        return self._min_component_cells

    def SetLinearInterpolator(self):
        """Back to the default interpolator (LinearInterpolateImageFunction<TImage, double>)."""
        self._bspline = None

    def Update(self):
        if self._input is None:
            # the ITK pipeline throws for a missing required input (txx:33)
            raise RuntimeError("CuberilleImageToMeshFilter: input 0 is required but not set")
        for attr, off, name, why in self._NOT_IN_A_GROUP:      # (before a device is touched)
            if len(self._devices) > 1 and getattr(self, attr) != off:
                raise _abi.CuberilleError(_abi.ERR_ARGUMENT, "%s is not offered in a group: %s" % (name, why))
        if self._band_on:
            # (before a device is touched: the four values against the input's pixel type)
            check_band(int(self._group_desc(self._input).pixel_type), self._band + self._band_values)
        if self._region is not None:
            # (before a device is touched: the box against the input's buffered region)
            check_region(self._group_desc(self._input), self._buffer_region(self._input))
        self._acquire(True)
        vol = self._input
        if self._step < 0.0:                      # txx:82-85, sticky like the reference (quirk Q3)
            self._step = max(vol.spacing) * 0.25
        prm = make_params(self._iso, self._triangles, self._project, self._threshold, self._step, self._relax,
                          self._max_steps, self._q1, self._variant, self._gradient)
        if len(self._devices) > 1 and not self._bspline and not self._stale_gradient and \
                not (self._project and self._gradient == GRADIENT_RECURSIVE_GAUSSIAN):
            if self._group is None:
                self._group = ExtractorGroup(self._devices)
            self._point_normals = None
            self._cell_pixels = None
            self._components = None
            self._point_scalars = None
            self.last_result = self._group.extract_host(vol, prm)
            self._output = self._group.download()
            self.last_number_of_slabs = len(self._group.plan(self._group_desc(vol), prm))
            return
        self._extractor.hold_gradient(self._stale_gradient)
        if self._bspline:
            self._extractor.set_interpolator(_abi.INTERP_BSPLINE, 3, *self._bspline)
        else:
            self._extractor.set_interpolator(_abi.INTERP_LINEAR)
        self._extractor.set_border(1 if self._pad_border else 0, self._border_pad_value)
        if self._region is not None:
            self._extractor.set_region(*self._buffer_region(vol))
        else:
            self._extractor.clear_region()
        if self._band_on:
            self._extractor.set_band(*(self._band + self._band_values))
        else:
            self._extractor.clear_band()
        self._extractor.set_point_normals(self._normals)
        self._point_normals = None
        self._extractor.set_cell_pixels(self._cell_pixels_on)
        self._cell_pixels = None
        keep = self._keep_largest or self._min_component_cells > 0
        self._extractor.set_components(self._components_on or keep)
        self._components = None
        if self._scalar_image is None:
            self._extractor.set_point_scalars(None)
        elif not self._scalar_uploaded:
            self._extractor.set_point_scalars(self._scalar_image, self._scalar_outside)
            self._scalar_uploaded = True
        self._point_scalars = None
        self.last_result = self._extractor.extract_host(vol, prm)
        # (the mesh is compacted on the device before anything of it comes to the host)
        if self._keep_largest:
            self._extractor.keep_components(_abi.KEEP_LARGEST)
        if self._min_component_cells > 0:
            self._extractor.keep_components(_abi.KEEP_MIN_CELLS, self._min_component_cells)
        self._output = self._extractor.download()
        if self._normals:
            self._point_normals = self._extractor.download_normals()
        if self._cell_pixels_on:
            self._cell_pixels = self._extractor.download_cell_pixels()
        if self._components_on or keep:
            self._components = self._extractor.download_components()
        if self._scalar_image is not None:
            self._point_scalars = self._extractor.download_point_scalars()
        self.last_number_of_slabs = 1

    @staticmethod
    def _group_desc(vol):
        return make_desc(vol.voxels.dtype, vol.dims, vol.spacing, vol.origin, vol.direction, getattr(vol, "index_start", (0, 0, 0)))

    def GetOutput(self):
        return self._output
