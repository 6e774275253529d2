// C-ABI host layer of the MI355X cuberille extractor (include/cuberille_hip.h).
//
// Plays the role of the body of itk::CuberilleImageToMeshFilter::GenerateData()
// (/root/reference/Source/itkCuberilleImageToMeshFilter.txx:59-216): resolves the
// parameters the way txx:75-95 does, then drives the HIP kernels of
// cuberille_kernels.hip on one stream.  No CPU fallback exists: without a gfx950
// device every computing entry point fails with CUBERILLE_ERR_NO_DEVICE.

#include "../../include/cuberille_hip.h"
#include "cuberille_internal.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <sys/mman.h>
#include <thread>
#include <utility>
#include <vector>

namespace cuberille {
// (cuberille_vtk.cpp, host code: the NORMALS block of cuberille_mesh_write_vtk)
int append_vtk_normals(const char *path, const float *normals, uint64_t n_points, int n_threads);
// (the CELL_DATA block: n_cells values of pixel_type, behind everything else in the file)
int append_vtk_cell_pixels(const char *path, const void *pixels, int pixel_type, uint64_t n_cells);
// (the component array of the POINT_DATA or the CELL_DATA block; block: "POINT_DATA" / "CELL_DATA" where this array opens the
//  block, null where the block exists)
int append_vtk_components(const char *path, const char *block, const uint32_t *labels, uint64_t n);
// (the point scalars' array, last in the POINT_DATA block; block as above)
int append_vtk_point_scalars(const char *path, const char *block, const double *values, uint64_t n);
}
using namespace cuberille;

namespace {

// text of the last failed cuberille_create on this thread (contexts are independent; so are their creators)
thread_local std::string g_create_error;

// Failure drill (cuberille_debug_set_option "fail_alloc_at" = n): the n-th device allocation this THREAD makes from now on
// reports out-of-memory without touching the device; -1 = off.  Lets the tests walk every allocation-failure path.
thread_local long long g_fail_alloc_countdown = -1;

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (g_fail_alloc_countdown >= 0 && g_fail_alloc_countdown-- == 0) return hipErrorOutOfMemory;
    if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
    // grow with head-room so that repeated calls on similar volumes do not re-allocate
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = want;
    return hipSuccess;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  // When the buffer has to grow anyway, grow it to `cover` -- what the NEXT extraction on the context will ask for when it is
  // launched from this one's sizes (cuberille_step_begin: + 25 %) -- so that the second extraction of a series does not
  // free and allocate the mesh buffers again (176 ms of one 14 ms extraction at 2048^3); back to `bytes` if that is too much.
  hipError_t reserve_covering(size_t bytes, size_t cover) {
    if (bytes <= cap) return hipSuccess;
    if (cover > bytes) {
      if (g_fail_alloc_countdown < 0) {          // (the failure drill counts one allocation per buffer: keep it so)
        const size_t had = cap;
        cap = 0;
        if (p) { (void)hipFree(p); p = nullptr; }
        if (hipMalloc(&p, cover + 256) == hipSuccess) { cap = cover + 256; return hipSuccess; }
        (void)hipGetLastError();
        p = nullptr;
        (void)had;
      }
    }
    return reserve(bytes);
  }
};

// Host memory of the context's own (cuberille_mesh_host): anonymous pages, 2 MiB aligned and advised as huge pages where
// the system has them; kept and re-used across extractions, grown with head-room.
struct HostBuf {
  void *p = nullptr, *base = nullptr;
  size_t cap = 0, mapped = 0;
  bool reserve(size_t bytes) {
    if (bytes <= cap) return true;
    release();
    const size_t huge = 2u << 20;
    size_t want = bytes + bytes / 8;
    want = (want + huge - 1) & ~(huge - 1);
    void *m = mmap(nullptr, want + huge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED) return false;
    base = m;
    mapped = want + huge;
    p = (void *)(((uintptr_t)m + huge - 1) & ~(uintptr_t)(huge - 1));
    cap = want;
#ifdef MADV_HUGEPAGE
    (void)madvise(p, cap, MADV_HUGEPAGE);
#endif
    return true;
  }
  void release() {
    if (base) (void)munmap(base, mapped);
    p = base = nullptr;
    cap = mapped = 0;
  }
};

// ---- the mesh's rows and the optional outputs (the attributes' words: kAttrWords, below enum Route) ----------
enum Attr { ATTR_NONE = -1, ATTR_NORMALS, ATTR_CELL_PIXELS, ATTR_COMPONENTS, N_ATTRS };
enum Row { ROW_POINTS, ROW_CELLS, ROW_NORMALS, ROW_CELL_PIX, ROW_COMP_POINT, ROW_COMP_CELL, ROW_COMP_COUNT, N_ROWS };
enum Per { PER_POINT, PER_CELL, PER_COMPONENT, N_PERS };
// A row: what it has one element of, that element's bytes, its attribute (ATTR_NONE: the mesh itself), and whether a
// reservation for no element still asks for one.  In the order an emit reserves them, and the keep their spare partners.
struct RowInfo { const char *name; Per per; size_t (*elem)(int verts_per_cell, size_t pixel); int attr; bool oneIfEmpty; };
const RowInfo kRows[N_ROWS] = {
    {"points", PER_POINT, [](int, size_t) { return 3 * sizeof(float); }, ATTR_NONE, false},
    {"cells", PER_CELL, [](int nv, size_t) { return (size_t)nv * sizeof(uint64_t); }, ATTR_NONE, true},
    {"normals", PER_POINT, [](int, size_t) { return 3 * sizeof(float); }, ATTR_NORMALS, false},
    {"cellPix", PER_CELL, [](int, size_t pixel) { return pixel; }, ATTR_CELL_PIXELS, true},
    {"compPoint", PER_POINT, [](int, size_t) { return sizeof(uint32_t); }, ATTR_COMPONENTS, false},
    {"compCell", PER_CELL, [](int, size_t) { return sizeof(uint32_t); }, ATTR_COMPONENTS, true},
    {"compCount", PER_COMPONENT, [](int, size_t) { return sizeof(uint64_t); }, ATTR_COMPONENTS, false},
};
const Per kAttrOf[N_ATTRS] = {PER_POINT, PER_CELL, PER_POINT};   // what an attribute hangs on: an emit with none of them reserves none of its rows
// The bytes a row of n[per] elements is reserved with (n: points, cells, components)
size_t row_reserve_bytes(int r, const u64 n[N_PERS], int verts_per_cell, size_t pixel) {
  const u64 have = n[kRows[r].per];
  return (size_t)(have || !kRows[r].oneIfEmpty ? have : 1) * kRows[r].elem(verts_per_cell, pixel);
}
struct MeshRow { DevBuf row, spare; };

// cuberille_set_point_scalars, the fourth optional output: a row held BESIDE the tables (the tables' sizes are
// written out in the host-only test of the three), with a {row, spare} pair and an {on, counting, have} state of its own and
// its own line wherever a loop over the tables stands for the others.  One double per point: the row of an emit of n points
// (none for an empty mesh), the spare of a keep to n.
size_t point_scalars_bytes(u64 n) { return (size_t)n * sizeof(double); }
struct PointScalars {
  bool on = false, counting = false, have = false;   // the setting, as the running count/emit pair found it, whether the last mesh has the row
  MeshRow rows;
  DevBuf copy;                       // CUBERILLE_MEM_HOST: the library's own copy of the second image
  const void *vox = nullptr;         // the second image on the device: the copy, or the caller's pointer (CUBERILLE_MEM_DEVICE)
  int pixel_type = 0, n[3] = {0, 0, 0};
  Geo geo{};
  double outside = 0.0;
};
const char *const kPointScalarsNoun = "point scalars", *const kPointScalarsFn = "cuberille_set_point_scalars";

}  // namespace

struct cuberille_ctx {
  int device = 0;
  hipStream_t own = nullptr, stream = nullptr;
  std::string err;
  DevBuf voxOwn, bits, flatBits, occ, prefix, segPre, blockTot, blockBase, cmap, headV, headQ, vqueue, escList;
  MeshRow rows[N_ROWS];                  // the mesh (kRows): an attribute's rows exist only while its setting is on, a spare behind a keep
  DevBuf &row(int r) { return rows[r].row; }
  DevBuf gradImg, rgA, rgB, rgScratch;   // gradient_variant 1: the gradient image and what its passes go through
  DevBuf heldGrad;                       // cuberille_hold_gradient: the float gradient image of the first projecting extraction
  HeldGradient held{};                   // ... with its geometry (img == null: none yet); what every later walk follows
  bool holdGradient = false;             // ... asked for
  double heldStep = -1.0;                // ... and the default step length that "filter object" resolved at its first extraction
  int interp = CUBERILLE_INTERP_LINEAR;  // cuberille_set_interpolator: the value interpolator of later walks ...
  int bsBits = 0;                        // ... and, for the B-spline, its coordinate / coefficient width (32 or 64)
  DevBuf bsCoef, bsScratch;              // the B-spline coefficient image, and the double scratch of its passes (32-bit only)
  // the three source-view settings, each as its setter left it; resolve_view makes one View of them per extraction
  int padWidth = 0;                      // cuberille_set_border: voxels of constant border implied around every later whole volume
  double padValue = 0.0;                 // ... and their value, which travels like the iso value
  long long padValueInt = 0;
  bool bandOn = false;                   // cuberille_set_band: every later whole-volume extraction meshes the binary image a band of the pixel values makes ...
  double bandV[4] = {0.0, 0.0, 0.0, 0.0};      // ... lower, upper, inside, outside, each travelling like the iso value
  long long bandVi[4] = {0, 0, 0, 0};
  bool regionOn = false;                 // cuberille_set_region: every later whole-volume extraction meshes this box of its buffer ...
  int64_t regionStart[3] = {0, 0, 0};    // ... its first voxel, as a position in the buffer (x, y, z) ...
  int64_t regionSize[3] = {0, 0, 0};     // ... and its size
  int bsValidBits = 0;                   // the coefficient image of the last B-spline extraction: its width (0: none) ...
  int64_t bsDims[3] = {0, 0, 0};         // ... and its size
  // the optional outputs (kAttrWords): the setting, the setting as the running count/emit pair found it, whether the last mesh has it
  struct { bool on = false, counting = false, have = false; } attr[N_ATTRS];
  PointScalars ps;                       // cuberille_set_point_scalars: beside the tables
  // the components' scratch, no rows of the mesh: the union-find's forest and the numbering's scan row (CompRows), and what
  // cuberille_keep_components decides and scans in; freed with the component rows
  DevBuf compParent, compScan, keepSel, keepScan, *const compScratch[4] = {&compParent, &compScan, &keepSel, &keepScan};
  u64 *hostK = nullptr;                  // K on its way to the host (pinned; allocated with the first extraction that has components on)
  u64 nComponents = 0;                   // ... K of the last mesh
  u64 *hostKeep = nullptr;               // cuberille_keep_components: K', n_points', n_cells' on their way to the host (pinned; allocated by the first call)
  hipEvent_t keepEv[2] = {};             // ... and the call's one event pair (created by the first call)
  HostBuf hostPoints, hostCells;         // cuberille_mesh_host: the last mesh in host memory of the context's own
  bool hostMeshValid = false;            // ... holds the mesh of the last emit
  Totals *hostTotals = nullptr;          // pinned
  uint32_t *hostOcc = nullptr;           // pinned mirror of the per-slice occupancy of the last slab count
  size_t hostOccCap = 0;
  hipEvent_t ev[8] = {};                 // the timing marks (enum Mark), recorded by mark()
  Tuning tune;                           // development switches (cuberille_debug_set_option)
  // overlapped ingestion (cuberille_extract_host): pinned staging ring and a copy stream
  hipStream_t copyStream = nullptr;
  void *stage[2] = {nullptr, nullptr};
  size_t stageBytes = 0;
  hipEvent_t stageFree[2] = {}, chunkIn[2] = {};
  int poolThreads = 0;                   // host threads of a chunked copy (StagePool); 0: the single-context rule.  A
                                         // cuberille_group splits that budget across its members
  bool aliasBelowBuffer = false;         // soft condition of the last slab count (cuberille_slab_info)
  bool aliasMustResolve = false;         // ... and it is certain: the source slice lies in this slab's own halo
  int aliasZ = -1;                       // local slice whose Q1 source is unresolved (the first occupied counted slice), -1
  bool slabMode = false;                 // the last count was given a slab
  bool thinHalo = false;                 // ... with CUBERILLE_SLAB_THIN_HALO: walks that leave the buffer are put aside
  bool pointsStartedEarly = false;       // split emit: the vertex phase ran ahead of the cells (two device intervals to add up)
  bool escapeChecked = false;            // THIN_HALO: the number of escaped walks of the current vertex phase has been read back
  // cuberille_step_begin / _end: what the previous extraction on this context produced sizes the blind launches
  bool warm = false;                     // cuberille_warm_up has run its toy extraction
  bool haveHistory = false;
  u64 histV = 0, histQ = 0;
  u32 histVW = 0;
  bool histDense = false;                // ... and whether a quarter or more of its words created vertices
  bool histShortWalks = false;           // ... and whether its walks took fewer than four passes per vertex on average
  int stepMode = 0;                      // 0: no step open; 1: launched blindly (sizes on the device); 2: sized by a host read;
                                         // 3: cuberille_step_classify has run, cuberille_step_count is next
  hipEvent_t voxelHaloEvent = nullptr;   // cuberille_step_count: the halo's VOXELS are complete behind this event of the
                                         // caller's (only the walk reads them; everything before it needs their bits alone)
  Totals *hostRows = nullptr;            // pinned: the gathered totals of all ranks, read back by cuberille_step_end
  size_t hostRowsCap = 0;
  u64 pointOffset = 0;                   // of the last emit
  const u64 *extIds = nullptr;           // cuberille_set_alias_plane: planes for the next emit (device pointers)
  const float *extPts = nullptr;
  // state of the last count
  bool counted = false, haveMesh = false, slabMesh = false;
  int countBsBits = 0;                   // the B-spline walk of the running count/emit pair: its width (0: not this interpolator)
  bool pointsEmitted = false;            // the offset-free part of the emit has been launched for the current count
  bool stagesTimed = false;              // the per-stage events of the running count/emit pair are being recorded
  bool lightTiming = false;              // a few million voxels at most: ONE event pair around the extraction (every event
                                         // between two kernels costs the stream about as much as such a volume's kernels)
  bool oneCall = false;                  // inside cuberille_extract_device: no host turn between count and emit, so three
                                         // events do (start, end of the pass, end): each one more idles the stream ~10 us
  Grid g{};
  Geo geo{};
  Params prm{};
  int pixel_type = 0;
  Workspace w{};
  size_t nwords = 0, nseg = 0;
  Totals tot{};
  cuberille_result res{};
};

namespace {

// The timing marks of an extraction, one event each (cuberille_ctx::ev); which a mode records: mark(), by finish_result.
enum Mark { PASS_BEGIN, CLASSIFY_END, PASS_END, CELLS_BEGIN, POINTS_BEGIN, POINTS_END, PROJECT_END, END };
hipError_t mark(cuberille_ctx *c, Mark m);

// every device buffer a context owns (cuberille_destroy frees them, cuberille_debug_device_bytes adds them up)
std::vector<DevBuf *> device_buffers(cuberille_ctx *c) {
  std::vector<DevBuf *> all = {&c->voxOwn, &c->bits, &c->flatBits, &c->occ, &c->prefix, &c->segPre, &c->blockTot, &c->blockBase,
                               &c->cmap, &c->headV, &c->headQ, &c->vqueue, &c->escList,
                               &c->gradImg, &c->rgA, &c->rgB, &c->rgScratch, &c->heldGrad, &c->bsCoef, &c->bsScratch};
  all.insert(all.end(), c->compScratch, c->compScratch + 4);
  for (MeshRow &m : c->rows) { all.push_back(&m.row); all.push_back(&m.spare); }
  // (the point scalars' three exist only while the setting is on -- off, its setter has released them and a failed call keeps
  //  none --; listed as well whenever one of them holds memory, so that nothing this context owns can go unlisted)
  if (c->ps.on || c->ps.rows.row.p || c->ps.rows.spare.p || c->ps.copy.p) {
    all.push_back(&c->ps.rows.row); all.push_back(&c->ps.rows.spare); all.push_back(&c->ps.copy);
  }
  return all;
}

// cuberille_set_components: the rows as their kernels take them
CompRows comp_rows(cuberille_ctx *c) {
  return {(u32 *)c->compParent.p, (u32 *)c->row(ROW_COMP_POINT).p, (u32 *)c->row(ROW_COMP_CELL).p, (u64 *)c->row(ROW_COMP_COUNT).p,
          c->compScan.p};
}

int fail(cuberille_ctx *c, int code, const std::string &msg) {
  if (c) c->err = msg; else g_create_error = msg;
  return code;
}

#define HIP_TRY(c, call)                                                                         \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      return fail((c), CUBERILLE_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));    \
  } while (0)

bool is_gfx950(int dev) {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess) return false;
  return std::strncmp(p.gcnArchName, "gfx950", 6) == 0;
}

size_t pixel_size(int pt) {
  switch (pt) {
    case CUBERILLE_PIX_U8: case CUBERILLE_PIX_I8: return 1;
    case CUBERILLE_PIX_U16: case CUBERILLE_PIX_I16: return 2;
    case CUBERILLE_PIX_U32: case CUBERILLE_PIX_I32: case CUBERILLE_PIX_F32: return 4;
    case CUBERILLE_PIX_F64: case CUBERILLE_PIX_I64: case CUBERILLE_PIX_U64: return 8;
  }
  return 0;
}

// The last mesh (as extracted, or as cuberille_keep_components left it): the bytes of a row -- what a download copies
size_t mesh_row_bytes(const cuberille_ctx *c, int r) {
  const u64 n[N_PERS] = {c->res.n_points, c->res.n_cells, c->nComponents};
  return (size_t)n[kRows[r].per] * kRows[r].elem(c->res.verts_per_cell, pixel_size(c->pixel_type));
}

// 3x3 inverse by cofactors (the parity tests hand the same matrix to the CPU checker, which
// uses the same formula; for the identity direction of every shipped volume it is exact)
void invert3(const double m[9], double inv[9]) {
  const double c00 = m[4] * m[8] - m[5] * m[7];
  const double c01 = m[5] * m[6] - m[3] * m[8];
  const double c02 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  inv[0] = c00 / det;
  inv[1] = (m[2] * m[7] - m[1] * m[8]) / det;
  inv[2] = (m[1] * m[5] - m[2] * m[4]) / det;
  inv[3] = c01 / det;
  inv[4] = (m[0] * m[8] - m[2] * m[6]) / det;
  inv[5] = (m[2] * m[3] - m[0] * m[5]) / det;
  inv[6] = c02 / det;
  inv[7] = (m[1] * m[6] - m[0] * m[7]) / det;
  inv[8] = (m[0] * m[4] - m[1] * m[3]) / det;
}

// cuberille_region_desc: the description of the box [start, start + size) of the buffer `img` describes -- what the reference
// is given after itk::ExtractImageFilter / RegionOfInterestImageFilter with the index kept: the box's size, its start index the
// buffer's plus the box's place in it, the same origin, spacing and direction.  The single validator of a box: the public symbol,
// resolve_view and cuberille_set_region come here.  *why: the text of a refusal.
int region_check(const cuberille_image_desc *img, const int64_t start[3], const int64_t size[3], cuberille_image_desc *out,
                 const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (!img || !out) { *why = "null image description"; return CUBERILLE_ERR_ARGUMENT; }
  if ((start == nullptr) != (size == nullptr)) { *why = "a region needs both its start and its size"; return CUBERILLE_ERR_ARGUMENT; }
  for (int i = 0; i < 3; i++)
    if (img->dims[i] < 1) { *why = "image dimensions must be >= 1"; return CUBERILLE_ERR_ARGUMENT; }
  if (!size || (size[0] == 0 && size[1] == 0 && size[2] == 0)) { *out = *img; return CUBERILLE_OK; }   // (off: the buffer itself)
  for (int i = 0; i < 3; i++) {
    if (start[i] < 0) { *why = "the region (cuberille_set_region) starts at a negative buffer position"; return CUBERILLE_ERR_ARGUMENT; }
    if (size[i] < 1) { *why = "the region (cuberille_set_region) must hold at least one voxel along every axis"; return CUBERILLE_ERR_ARGUMENT; }
    if (start[i] > img->dims[i] || size[i] > img->dims[i] - start[i]) {
      *why = "the region (cuberille_set_region) leaves the buffer";
      return CUBERILLE_ERR_ARGUMENT;
    }
  }
  cuberille_image_desc d = *img;
  for (int i = 0; i < 3; i++) {
    // (a box inside the buffer: its size passes the limit on dims when the buffer's does)
    if (img->dims[i] > 0x7fffffffLL) { *why = "image dimension exceeds 2^31-1"; return CUBERILLE_ERR_LIMIT; }
    if (img->index_start[i] < -(1LL << 30) || img->index_start[i] > (1LL << 30)) {
      *why = "the buffered region's start index must lie within +-2^30";
      return CUBERILLE_ERR_LIMIT;
    }
    const int64_t at = img->index_start[i] + start[i];
    if (at < -(1LL << 30) || at > (1LL << 30)) { *why = "the region's start index (the buffer's + the box's) must lie within +-2^30"; return CUBERILLE_ERR_LIMIT; }
    // the kernels add the start index and a position in `int`: the index one past the box's last, and the one before its first
    if (at + size[i] > 0x7fffffffLL || at - 1 < -0x80000000LL) {
      *why = "the region's start index + size exceeds 2^31-1";
      return CUBERILLE_ERR_LIMIT;
    }
    d.dims[i] = size[i];
    d.index_start[i] = at;
  }
  *out = d;
  return CUBERILLE_OK;
}

// cuberille_band_check: lower, upper, inside, outside against a pixel type.  All four are values OF the pixel type in
// itk::BinaryThresholdImageFilter<Image<T>, Image<T>>: each must be one the type holds -- an integer type takes no fraction and
// nothing beyond its range (the window of the iso and the ring value, lo - 1 < v < hi + 1, with the fraction refused as well: a
// bound cut off like a C cast would move the band by a label); the 64-bit integer types are judged by the double for the range
// and carry the value in vi -- and the filter throws for lower > upper.  A NaN bound is refused for the floating types too:
// it makes an empty band by accident.  The floating types convert a double like the iso value does (a C cast), and NaN and
// infinite VALUES are a float image's to hold.
int band_check(int pixel_type, const double v[4], const int64_t vi[4], const char **why) {
  static const char *const names[4] = {"lower bound", "upper bound", "inside value", "outside value"};
  static thread_local std::string text;
  auto no = [&](const std::string &m) { text = "band (cuberille_set_band): " + m; if (why) *why = text.c_str(); return CUBERILLE_ERR_ARGUMENT; };
  if (pixel_size(pixel_type) == 0) return no("unknown pixel type");
  if (!v || !vi) return no("null value pointer");
  double lo = 0.0, hi = 0.0;
  bool integer = true, wide = false;
  switch (pixel_type) {
    case CUBERILLE_PIX_U8: hi = 255.0; break;
    case CUBERILLE_PIX_I8: lo = -128.0; hi = 127.0; break;
    case CUBERILLE_PIX_U16: hi = 65535.0; break;
    case CUBERILLE_PIX_I16: lo = -32768.0; hi = 32767.0; break;
    case CUBERILLE_PIX_U32: hi = 4294967295.0; break;
    case CUBERILLE_PIX_I32: lo = -2147483648.0; hi = 2147483647.0; break;
    case CUBERILLE_PIX_I64: lo = -9223372036854775808.0; hi = 9223372036854775808.0; wide = true; break;      // [lo, hi)
    case CUBERILLE_PIX_U64: lo = 0.0; hi = 18446744073709551616.0; wide = true; break;
    default: integer = false; break;
  }
  for (int k = 0; k < 4; k++) {
    if (integer) {
      // (a 64-bit value rounds as a double -- one just under the type's top UP to it, one just below an int64's bottom up
      //  to that: vi, which wraps what the type does not hold to its other end, tells them apart by its sign)
      const bool atTop = wide && v[k] == hi && (pixel_type == CUBERILLE_PIX_I64 ? vi[k] > 0 : vi[k] < 0);
      const bool wrapped = pixel_type == CUBERILLE_PIX_I64 && ((v[k] < 0.0 && vi[k] >= 0) || (v[k] > 0.0 && vi[k] <= 0));
      const bool inRange = wide ? (v[k] >= lo && (v[k] < hi || atTop) && !wrapped) : (v[k] > lo - 1.0 && v[k] < hi + 1.0);
      if (!inRange || v[k] != std::floor(v[k])) return no(std::string("the ") + names[k] + " is not representable in the pixel type");
    } else if (k < 2 && v[k] != v[k]) {
      return no(std::string("the ") + names[k] + " is NaN");
    }
  }
  bool ordered;
  if (pixel_type == CUBERILLE_PIX_U64) ordered = (uint64_t)vi[0] <= (uint64_t)vi[1];
  else if (pixel_type == CUBERILLE_PIX_I64) ordered = vi[0] <= vi[1];
  else ordered = v[0] <= v[1];
  if (!ordered) return no("the lower bound is above the upper bound (itk::BinaryThresholdImageFilter throws there)");
  return CUBERILLE_OK;
}

// Does a value that travels as a double (the iso value, the ring's) convert to the pixel type without leaving its range?  (The
// 8- to 32-bit integer types; a fraction is cut off like a C cast does.  The other types take any double.)
bool converts(int pixel_type, double v) {
  double lo = 0.0, hi = 0.0;
  switch (pixel_type) {
    case CUBERILLE_PIX_U8: hi = 255.0; break;
    case CUBERILLE_PIX_I8: lo = -128.0; hi = 127.0; break;
    case CUBERILLE_PIX_U16: hi = 65535.0; break;
    case CUBERILLE_PIX_I16: lo = -32768.0; hi = 32767.0; break;
    case CUBERILLE_PIX_U32: hi = 4294967295.0; break;
    case CUBERILLE_PIX_I32: lo = -2147483648.0; hi = 2147483647.0; break;
    default: break;
  }
  return hi == lo || (v > lo - 1.0 && v < hi + 1.0);
}

// The entry points that differ in what they offer of a setting (the source views: resolve_view; point normals: validate).
// ROUTE_HOST: cuberille_extract_host, which uploads a box alone.  ROUTE_WARM_UP only reserves: it looks at what changes a size
// (the border, the region), not at the band nor at the parameters.
enum Route { ROUTE_DEVICE, ROUTE_HOST, ROUTE_SLAB, ROUTE_STEP, ROUTE_STREAM, ROUTE_GROUP, ROUTE_WARM_UP, N_ROUTES };

// (an all-zero slab stands for the whole volume)
bool whole_volume(const cuberille_slab *slab) {
  return !slab || (slab->global_nz == 0 && slab->z_begin == 0 && slab->own_z0 == 0 && slab->own_z1 == 0);
}

// What is said of an attribute (modelled on kViewWords): its name in words and as the C setter.  Every attribute describes ONE
// context's whole volume, so why a route does not offer it (null: offered) and why a slab does not is said once for all.
const struct { const char *noun, *fn; } kAttrWords[N_ATTRS] = {
    {"point normals", "cuberille_set_point_normals"}, {"cell pixels", "cuberille_set_cell_pixels"}, {"components", "cuberille_set_components"}};
const char *const kAttrRoute[N_ROUTES] = {nullptr, nullptr, nullptr, " belong to one context's whole volume: not offered with the cuberille_step_* calls",
                                          nullptr, "they belong to one context's whole volume, not offered in a group", nullptr};
const char *const kAttrSlab = " belong to a whole volume: not offered on slabs";
std::string attr_missing(int a) { return std::string("no ") + kAttrWords[a].noun + ": the last extraction ran with the setting off (" + kAttrWords[a].fn + ")"; }

// Is every attribute that is on offered to an extraction on this route, with these parameters (null: not looked at), of this
// slab of a buffer of nz slices (null or all zero: the whole volume; a slab that is the whole buffer passes)?  CUBERILLE_OK, or
// the first refusal with its text in *why.  No device is touched.
int attrs_offered(const cuberille_ctx *c, const cuberille_params *prm, Route route, const cuberille_slab *slab, int64_t nz, const char **why) {
  static thread_local std::string text;
  auto no = [&](const std::string &m) { text = m; *why = text.c_str(); return CUBERILLE_ERR_ARGUMENT; };
  *why = "";
  for (int a = 0; a < N_ATTRS; a++) {
    if (!c->attr[a].on) continue;
    const std::string noun = kAttrWords[a].noun, fn = kAttrWords[a].fn, name = noun + " (" + fn + ")";
    if (const char *r = kAttrRoute[route]) return route == ROUTE_GROUP ? no("has " + noun + " set (" + fn + "): " + r) : no(name + r);
    if (a == ATTR_NORMALS && prm) {   // one definition, the central-difference gradient of the CURRENT whole volume at the final vertex
      if (c->holdGradient)
        return no(name + " are not offered on a context holding a gradient (cuberille_hold_gradient): the reference would evaluate the stale image there");
      if (prm->gradient_variant != CUBERILLE_GRADIENT_CENTRAL)
        return no(name + " are the central-difference gradient: not offered with CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN");
    }
    if (!whole_volume(slab) && (slab->global_nz != nz || slab->own_z0 != slab->z_begin || slab->own_z1 != slab->z_begin + nz)) return no(name + kAttrSlab);
  }
  if (c->ps.on) {                     // the point scalars, beside the table: one context's whole volume like the three, in their words
    const std::string noun = kPointScalarsNoun, fn = kPointScalarsFn, name = noun + " (" + fn + ")";
    if (const char *r = kAttrRoute[route]) return route == ROUTE_GROUP ? no("has " + noun + " set (" + fn + "): " + r) : no(name + r);
    if (!whole_volume(slab) && (slab->global_nz != nz || slab->own_z0 != slab->z_begin || slab->own_z1 != slab->z_begin + nz)) return no(name + kAttrSlab);
  }
  return CUBERILLE_OK;
}

int validate(cuberille_ctx *c, const cuberille_image_desc *img, const void *vox, const cuberille_params *prm, Route route = ROUTE_DEVICE) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (!img || !vox || !prm) return fail(c, CUBERILLE_ERR_ARGUMENT, "null image, voxel or parameter pointer");
  if (pixel_size(img->pixel_type) == 0) return fail(c, CUBERILLE_ERR_ARGUMENT, "unknown pixel type");
  for (int i = 0; i < 3; i++) {
    if (img->dims[i] < 1) return fail(c, CUBERILLE_ERR_ARGUMENT, "image dimensions must be >= 1");
    if (img->dims[i] > 0x7fffffffLL) return fail(c, CUBERILLE_ERR_LIMIT, "image dimension exceeds 2^31-1");
    if (!(img->spacing[i] > 0.0)) return fail(c, CUBERILLE_ERR_ARGUMENT, "spacing must be > 0");
    if (img->index_start[i] < -(1LL << 30) || img->index_start[i] > (1LL << 30))
      return fail(c, CUBERILLE_ERR_LIMIT, "the buffered region's start index must lie within +-2^30");
  }
  if (prm->projection_variant < CUBERILLE_PROJECT_DEFAULT || prm->projection_variant > CUBERILLE_PROJECT_LINESEARCH)
    return fail(c, CUBERILLE_ERR_ARGUMENT, "unknown projection variant");
  if (prm->gradient_variant < CUBERILLE_GRADIENT_CENTRAL || prm->gradient_variant > CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN)
    return fail(c, CUBERILLE_ERR_ARGUMENT, "unknown gradient variant");
  if (prm->gradient_variant == CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN && prm->project_vertices && c->holdGradient)
    return fail(c, CUBERILLE_ERR_ARGUMENT, "cuberille_hold_gradient holds the central-difference gradient image the reference ships: not offered with the recursive-Gaussian one");
  if (prm->gradient_variant == CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN && prm->project_vertices)
    for (int i = 0; i < 3; i++)
      if (img->dims[i] < 4)   // (ITK's recursive filter throws for shorter lines)
        return fail(c, CUBERILLE_ERR_ARGUMENT, "the recursive-Gaussian gradient needs at least 4 voxels along every axis");
  if (c->interp == CUBERILLE_INTERP_BSPLINE && prm->project_vertices) {
    if (prm->projection_variant != CUBERILLE_PROJECT_DEFAULT)
      return fail(c, CUBERILLE_ERR_ARGUMENT, "the B-spline interpolator walks the default projection branch only (txx:439-474)");
    if (prm->gradient_variant != CUBERILLE_GRADIENT_CENTRAL)
      return fail(c, CUBERILLE_ERR_ARGUMENT, "the B-spline interpolator is offered with the central-difference gradient only");
    if (c->holdGradient)
      return fail(c, CUBERILLE_ERR_ARGUMENT, "the B-spline interpolator is not offered on a context holding a gradient (cuberille_hold_gradient)");
  }
  // the optional outputs against the route (a slab that is not the whole volume: count_prepare)
  const char *why = "";
  if (const int rc = attrs_offered(c, prm, route, nullptr, 0, &why)) return fail(c, rc, why);
  // the iso value is an InputPixelType in the reference (h:180-181)
  if (!converts(img->pixel_type, prm->iso_value))
    return fail(c, CUBERILLE_ERR_ARGUMENT, "iso value is not representable in the pixel type");
  return CUBERILLE_OK;
}

}  // namespace

extern "C" {

int cuberille_region_desc(const cuberille_image_desc *img, const int64_t start[3], const int64_t size[3], cuberille_image_desc *cropped) {
  const char *why = "";
  const int rc = region_check(img, start, size, cropped, &why);
  if (rc) g_create_error = why;     // (no context to keep the text: cuberille_last_error(NULL), per thread like a failed create's)
  return rc;
}

int cuberille_abi_version(void) { return CUBERILLE_ABI_VERSION; }

int cuberille_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int d = 0; d < n; d++) if (is_gfx950(d)) ok++;
  return ok;
}

const char *cuberille_last_error(const cuberille_ctx *ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int cuberille_create(cuberille_ctx **out, int device_id) {
  if (!out) return fail(nullptr, CUBERILLE_ERR_ARGUMENT, "null output pointer");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(nullptr, CUBERILLE_ERR_NO_DEVICE, "no HIP device: the cuberille hot path has no CPU fallback");
  if (device_id < 0 || device_id >= n) return fail(nullptr, CUBERILLE_ERR_ARGUMENT, "device id out of range");
  if (!is_gfx950(device_id))
    return fail(nullptr, CUBERILLE_ERR_NO_DEVICE, "device is not gfx950 (MI355X); this library carries gfx950 code only");
  cuberille_ctx *c = new (std::nothrow) cuberille_ctx;
  if (!c) return fail(nullptr, CUBERILLE_ERR_ARGUMENT, "out of host memory");
  c->device = device_id;
  hipError_t e = hipSetDevice(device_id);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipHostMalloc((void **)&c->hostTotals, sizeof(Totals), hipHostMallocDefault);
  for (int i = 0; i < 8 && e == hipSuccess; i++) e = hipEventCreate(&c->ev[i]);
  if (e != hipSuccess) {
    g_create_error = std::string("cuberille_create: ") + hipGetErrorString(e);
    cuberille_destroy(c);
    return CUBERILLE_ERR_HIP;
  }
  c->stream = c->own;
  *out = c;
  return CUBERILLE_OK;
}

void cuberille_destroy(cuberille_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->own) (void)hipStreamSynchronize(c->own);
  if (c->copyStream) (void)hipStreamSynchronize(c->copyStream);
  for (DevBuf *b : device_buffers(c)) b->release();
  c->hostPoints.release();
  c->hostCells.release();
  if (c->hostTotals) (void)hipHostFree(c->hostTotals);
  if (c->hostOcc) (void)hipHostFree(c->hostOcc);
  if (c->hostRows) (void)hipHostFree(c->hostRows);
  if (c->hostK) (void)hipHostFree(c->hostK);
  if (c->hostKeep) (void)hipHostFree(c->hostKeep);
  for (int i = 0; i < 2; i++) if (c->keepEv[i]) (void)hipEventDestroy(c->keepEv[i]);
  for (int i = 0; i < 2; i++) {
    if (c->stage[i]) (void)hipHostFree(c->stage[i]);
    if (c->stageFree[i]) (void)hipEventDestroy(c->stageFree[i]);
    if (c->chunkIn[i]) (void)hipEventDestroy(c->chunkIn[i]);
  }
  for (int i = 0; i < 8; i++) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  if (c->copyStream) (void)hipStreamDestroy(c->copyStream);
  if (c->own) (void)hipStreamDestroy(c->own);
  delete c;
}

int cuberille_set_stream(cuberille_ctx *c, void *hip_stream) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own;
  return CUBERILLE_OK;
}

}  // extern "C"

namespace {

// How far, in slices, the projection can carry a vertex away from the slice it was created in, plus the cell's
// upper neighbour, the gradient ring and rounding: what a slab must hold beyond its owned range on each side.
// The walk moves at most step * sum(relax^k, k = 0 .. max_steps+1) in physical space (txx:449-470); the row of
// PhysicalPointToIndex for z turns that into slices.
long long projection_reach(const Geo &geo, const Params &p) {
  if (!p.project) return 0;
  const double n = (double)p.max_steps + 2.0;
  double travel;
  if (p.relax >= 1.0) travel = p.step * n;
  else if (p.relax <= 0.0) travel = p.step;
  else travel = p.step * (1.0 - std::pow(p.relax, n)) / (1.0 - p.relax);
  const double rowNorm = std::sqrt(geo.p2i[6] * geo.p2i[6] + geo.p2i[7] * geo.p2i[7] + geo.p2i[8] * geo.p2i[8]);
  // Where the walk STARTS: the reference moves the corner's index position to physical space and takes half a spacing off
  // every PHYSICAL axis (txx:266-270) -- half a voxel back along every index axis only while the direction matrix is the
  // identity.  Under a tilted direction the start lies row_z(PhysicalPointToIndex) . spacing/2 slices below the corner's
  // index instead of 1/2: with spacing (3, 1.7, 0.25) up to ten slices away from the lattice corner (found by
  // tests/fuzz_campaign.py, round 5: slabs cut to the old figure clamped four walks of a 19-slice volume).
  const double startOff = (geo.p2i[6] * geo.spacing[0] + geo.p2i[7] * geo.spacing[1] + geo.p2i[8] * geo.spacing[2]) * 0.5;
  const double astray = std::fabs(startOff - 0.5);
  const double slices = std::ceil(travel * rowNorm) + (astray < 1e-9 ? 0.0 : std::ceil(astray));
  if (!(slices < 1e9)) return 1000000000LL;
  return (long long)slices + 3;
}

void resolve(const cuberille_image_desc *img, const cuberille_params *prm, Geo &geo, Params &p) {
  // geometry and parameters (txx:75-85)
  double maxSpacing = img->spacing[0];
  for (int i = 0; i < 3; i++) {
    geo.spacing[i] = img->spacing[i];
    geo.origin[i] = img->origin[i];
    geo.gcoef[i] = (float)(0.5 * (1.0 / img->spacing[i]));
    geo.istart[i] = (int)img->index_start[i];
    if (img->spacing[i] > maxSpacing) maxSpacing = img->spacing[i];
  }
  for (int i = 0; i < 9; i++) geo.dir[i] = img->direction[i];
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) geo.i2p[r * 3 + k] = geo.dir[r * 3 + k] * geo.spacing[k];
  invert3(geo.i2p, geo.p2i);
  p.iso = prm->iso_value;
  p.isoInt = (long long)prm->iso_value_int;
  if (img->pixel_type == CUBERILLE_PIX_I64) p.iso = (double)prm->iso_value_int;          // what the walk compares with
  if (img->pixel_type == CUBERILLE_PIX_U64) p.iso = (double)(uint64_t)prm->iso_value_int;
  p.thr = prm->distance_threshold;
  p.step = prm->step_length < 0.0 ? maxSpacing * 0.25 : prm->step_length;
  p.relax = prm->relaxation;
  p.max_steps = prm->max_steps;
  p.triangles = prm->generate_triangles != 0;
  p.project = prm->project_vertices != 0;
  p.q1 = prm->emulate_empty_slice_aliasing != 0;
  p.variant = prm->projection_variant;
  p.gradVariant = prm->gradient_variant;
}

// ---- source views: cuberille_set_border, cuberille_set_region and cuberille_set_band as one kind of setting -----------------
// (the entry points that differ in what they offer of a view: enum Route, above validate)

// The one table of what is not offered: per kind its name in words and as the C function, the reason per route (null: offered)
// and what a second image of the view's shape -- B-spline coefficients, a gradient image -- would have to be.
struct ViewWords {
  const char *noun, *fn;
  const char *route[N_ROUTES];
  const char *second;
};
const ViewWords kViewWords[4] = {
    {"", "", {}, ""},
    {"an implied border", "cuberille_set_border",
     {nullptr, nullptr, " belongs to a whole volume: not offered on slabs",
      " would have to reach across ranks: not offered with the cuberille_step_* calls", nullptr,
      "the ring would have to reach across slabs, not offered in a group", nullptr},
     "need the ring"},
    {"a region", "cuberille_set_region",
     {nullptr, nullptr, " is a box of a whole volume: not offered on slabs",
      " is a box of one context's whole volume: not offered with the cuberille_step_* calls",
      " is not offered with cuberille_extract_stream: the source produces whole slices",
      "a box of one context's whole volume, not offered in a group", nullptr},
     "be the box's"},
    {"a band", "cuberille_set_band",
     {nullptr, nullptr, " belongs to a whole volume: not offered on slabs",
      " belongs to one context's whole volume: not offered with the cuberille_step_* calls",
      " is not offered with cuberille_extract_stream", "it belongs to one context's whole volume, not offered in a group", nullptr},
     "be the binary image's"},
};
// ... and why two of them do not go together, [the later kind][the earlier one]
const char *const kViewPairs[4][4] = {
    {}, {},
    {nullptr, "the box's faces inside the buffer would need a ring of their own"},
    {nullptr, "the ring's value would have to be one of the band's two", "the pitched sweep and walk have no band form"},
};

// cuberille_set_border against an image: the limits of validate() hold for the image with its ring, and the ring's value converts
// like the iso value (a fraction is cut off like a C cast does, the range is the pixel type's)
int border_check(const cuberille_image_desc *img, int padWidth, double padValue, bool value, const char **why) {
  for (int i = 0; i < 3; i++) {
    if (img->dims[i] + 2 * padWidth > 0x7fffffffLL) { *why = "image dimension with its border exceeds 2^31-1"; return CUBERILLE_ERR_LIMIT; }
    if (img->index_start[i] - padWidth < -(1LL << 30)) { *why = "the bordered region's start index must lie within +-2^30"; return CUBERILLE_ERR_LIMIT; }
  }
  if (value && !converts(img->pixel_type, padValue)) {
    *why = "the border value (cuberille_set_border) is not representable in the pixel type";
    return CUBERILLE_ERR_ARGUMENT;
  }
  return CUBERILLE_OK;
}

// The frame the layout, the geometry and every workspace size follow from -- what the reference would be handed: the caller's
// image; with its ring (after itk::ConstantPadImageFilter: the region grown by one on every side, its start index moved down by
// one); or cut to its box (cuberille_region_desc); origin, spacing and direction the same.  The sweep and the walk alone read
// the caller's buffer.
cuberille_image_desc framed_desc(const View &v, const cuberille_image_desc *img) {
  cuberille_image_desc d = *img;
  if (v.kind == VIEW_BORDER)
    for (int i = 0; i < 3; i++) { d.dims[i] += 2; d.index_start[i] -= 1; }
  if (v.kind == VIEW_REGION) {
    const int64_t start[3] = {v.start[0], v.start[1], v.start[2]}, size[3] = {v.size[0], v.size[1], v.size[2]};
    if (region_check(img, start, size, &d, nullptr) != CUBERILLE_OK) return *img;     // (resolve_view has passed the box)
  }
  return d;
}

// A region whose box has been uploaded on its own (cuberille_extract_host): `box` describes the device copy, contiguous, the
// pitches are the box's -- what is left of the view is the walk's runtime start index
View applied_region(const cuberille_image_desc &box) {
  View v{};
  v.kind = VIEW_REGION;
  for (int i = 0; i < 3; i++) v.size[i] = box.dims[i];
  v.rowPitch = box.dims[0]; v.slicePitch = box.dims[0] * box.dims[1];
  return v;
}

// What of the parameters a view's refusals depend on (resolve() fills the rest, from the frame)
Params projection_features(const cuberille_params *prm) {
  Params p{};
  p.project = prm->project_vertices != 0;
  p.variant = prm->projection_variant;
  p.gradVariant = prm->gradient_variant;
  return p;
}

// The settings of a context against an image on a route: one View, or a refusal with its text in *why.  Every "not offered"
// comes from here: the route's (kViewWords), two settings at once (kViewPairs), each setting's validator, what the projection
// would need a second image for.  No device is touched.
int resolve_view(const cuberille_ctx *c, const cuberille_image_desc *img, const Params &p, Route route, View *out, const char **why) {
  static thread_local std::string text;
  auto no = [&](const std::string &m) { text = m; *why = text.c_str(); return CUBERILLE_ERR_ARGUMENT; };
  auto name = [](int k) { return std::string(kViewWords[k].noun) + " (" + kViewWords[k].fn + ")"; };
  const bool on[4] = {false, c->padWidth != 0, c->regionOn, c->bandOn && route != ROUTE_WARM_UP};
  View v{};
  *why = "";
  for (int k = VIEW_BORDER; k <= VIEW_BAND; k++) {
    if (!on[k]) continue;
    if (const char *r = kViewWords[k].route[route])
      return route == ROUTE_GROUP ? no(std::string("has ") + kViewWords[k].noun + " set (" + kViewWords[k].fn + "): " + r) : no(name(k) + r);
    for (int j = VIEW_BORDER; j < k; j++)
      if (on[j]) return no(name(k) + " together with " + name(j) + " is not offered: " + kViewPairs[k][j]);
    v.kind = k;
  }
  int rc = CUBERILLE_OK;
  cuberille_image_desc framed = *img;
  if (v.kind == VIEW_BORDER) {
    v.padValue = c->padValue; v.padValueInt = c->padValueInt;
    rc = border_check(img, c->padWidth, c->padValue, route != ROUTE_WARM_UP, why);
  } else if (v.kind == VIEW_REGION) {
    for (int i = 0; i < 3; i++) { v.start[i] = c->regionStart[i]; v.size[i] = c->regionSize[i]; }
    rc = region_check(img, c->regionStart, c->regionSize, &framed, why);
    v.pitched = framed.dims[0] != img->dims[0] || framed.dims[1] != img->dims[1];
  } else if (v.kind == VIEW_BAND) {
    for (int k = 0; k < 4; k++) { v.bandV[k] = c->bandV[k]; v.bandVi[k] = c->bandVi[k]; }
    rc = band_check(img->pixel_type, c->bandV, (const int64_t *)c->bandVi, why);
  }
  if (rc) return rc;
  // (the box's rows and slices lie the BUFFER's pitches apart; every other view's the frame's own)
  if (v.kind == VIEW_BORDER) framed = framed_desc(v, img);
  const cuberille_image_desc *mem = v.kind == VIEW_REGION ? img : &framed;
  v.rowPitch = mem->dims[0]; v.slicePitch = mem->dims[0] * mem->dims[1];
  if (v.kind != VIEW_WHOLE && p.project && route != ROUTE_WARM_UP) {
    if (c->interp == CUBERILLE_INTERP_BSPLINE)
      return no(name(v.kind) + " is not offered with the B-spline interpolator: its coefficient image would " + kViewWords[v.kind].second);
    if (c->holdGradient) return no(name(v.kind) + " is not offered on a context holding a gradient image (cuberille_hold_gradient)");
    if (p.gradVariant != CUBERILLE_GRADIENT_CENTRAL)
      return no(name(v.kind) + " is offered with the central-difference gradient only: the recursive-Gaussian gradient image would " + kViewWords[v.kind].second);
    if (p.variant != CUBERILLE_PROJECT_DEFAULT) return no(name(v.kind) + " is offered with the default projection branch only (txx:439-474)");
  }
  *out = v;
  return CUBERILLE_OK;
}

// resolve_view for an entry point: the refusal becomes the context's error
int view_of(cuberille_ctx *c, const cuberille_image_desc *img, const cuberille_params *prm, Route route, View *v) {
  const char *why = "";
  const int rc = resolve_view(c, img, projection_features(prm), route, v, &why);
  return rc ? fail(c, rc, why) : CUBERILLE_OK;
}

// RecursiveGaussianImageFilter::SetUp of ITK 3.x (Deriche's fourth-order recursive Gaussian): the 20 coefficients of one
// separable pass -- order 0 smoothing, order 1 first derivative with NormalizeAcrossScale (txx:490) -- for `sigma` in
// physical units on an axis of the given spacing.  Evaluated on the host in double, once per extraction; the kernels
// (k_rg_pass) only run the recurrences.  Layout = cuberille::DericheCoef.
void deriche_setup(double sigma, double spacing, int order, double out[20]) {
  static const double A1[2] = {1.3530, -0.6724}, B1[2] = {1.8151, -3.4327}, W1 = 0.6681, L1 = -1.3932;
  static const double A2[2] = {-0.3531, 0.6724}, B2[2] = {0.0902, 0.6100}, W2 = 2.0787, L2 = -1.3732;
  const double sigmad = sigma / spacing;
  const double cos1 = std::cos(W1 / sigmad), cos2 = std::cos(W2 / sigmad), sin1 = std::sin(W1 / sigmad), sin2 = std::sin(W2 / sigmad);
  const double exp1 = std::exp(L1 / sigmad), exp2 = std::exp(L2 / sigmad);
  double D4 = exp1 * exp1 * exp2 * exp2;
  double D3 = -2 * cos1 * exp1 * exp2 * exp2;
  D3 += -2 * cos2 * exp2 * exp1 * exp1;
  double D2 = 4 * cos2 * cos1 * exp1 * exp2;
  D2 += exp1 * exp1 + exp2 * exp2;
  const double D1 = -2 * (exp2 * cos2 + exp1 * cos1);
  const double SD = 1.0 + D1 + D2 + D3 + D4;
  const double DD = D1 + 2 * D2 + 3 * D3 + 4 * D4;
  const double a1 = A1[order], b1 = B1[order], a2 = A2[order], b2 = B2[order];
  double N0 = a1 + a2;
  double N1 = exp2 * (b2 * sin2 - (a2 + 2 * a1) * cos2);
  N1 += exp1 * (b1 * sin1 - (a1 + 2 * a2) * cos1);
  double N2 = (a1 + a2) * cos2 * cos1;
  N2 -= b1 * cos2 * sin1 + b2 * cos1 * sin2;
  N2 *= 2 * exp1 * exp2;
  N2 += a2 * exp1 * exp1 + a1 * exp2 * exp2;
  double N3 = exp2 * exp1 * exp1 * (b2 * sin2 - a2 * cos2);
  N3 += exp1 * exp2 * exp2 * (b1 * sin1 - a1 * cos1);
  const double SN = N0 + N1 + N2 + N3;
  const double DN = N1 + 2 * N2 + 3 * N3;
  double M1, M2, M3, M4;
  if (order == 0) {
    const double alpha0 = 2 * SN / SD - N0;
    N0 /= alpha0; N1 /= alpha0; N2 /= alpha0; N3 /= alpha0;
    M1 = N1 - D1 * N0; M2 = N2 - D2 * N0; M3 = N3 - D3 * N0; M4 = -D4 * N0;
  } else {
    double alpha1 = 2 * (SN * DD - DN * SD) / (SD * SD);
    alpha1 *= 1.0;                                // (spacing is positive here: no sign flip)
    N0 *= sigma / alpha1; N1 *= sigma / alpha1; N2 *= sigma / alpha1; N3 *= sigma / alpha1;
    M1 = -(N1 - D1 * N0); M2 = -(N2 - D2 * N0); M3 = -(N3 - D3 * N0); M4 = D4 * N0;
  }
  const double sn = N0 + N1 + N2 + N3, sm = M1 + M2 + M3 + M4, sd = 1.0 + D1 + D2 + D3 + D4;
  const double v[20] = {N0, N1, N2, N3, D1, D2, D3, D4, M1, M2, M3, M4,
                        D1 * sn / sd, D2 * sn / sd, D3 * sn / sd, D4 * sn / sd, D1 * sm / sd, D2 * sm / sd, D3 * sm / sd, D4 * sm / sd};
  for (int i = 0; i < 20; i++) out[i] = v[i];
}

// BSplineDecompositionImageFilter of ITK 3.x, order 3 (one pole), for a line of n pixels: SetPoles, the gain of
// DataToCoefficients1D, the horizon of SetInitialCausalCoefficient (m_Tolerance 1e-10) and the powers its full mirror sum
// and SetInitialAntiCausalCoefficient use -- in double on the host, with the host's pow / log, like the restatement in
// itk/itk_lite/itkBSplineLite.h.  Layout = cuberille::BsAxis; the kernels (k_bs_rows, k_bs_lines) run the recurrences.
BsAxis bspline_axis(long long n) {
  BsAxis a{};
  a.z = std::sqrt(3.0) - 2.0;
  double c0 = 1.0;
  c0 = c0 * (1.0 - a.z) * (1.0 - 1.0 / a.z);
  a.gain = c0;
  a.iz = 1.0 / a.z;
  a.zN1 = std::pow(a.z, (double)(n - 1LL));
  a.anti = a.z / (a.z * a.z - 1.0);
  a.horizon = (int)(long)std::ceil(std::log(1e-10) / std::log(std::fabs(a.z)));
  a.n = n;
  return a;
}

// The layout of a whole image (count_prepare narrows it to a slab's owned range).
Grid whole_grid(const cuberille_image_desc *img, const Tuning &t) {
  Grid g{};
  g.nx = (int)img->dims[0]; g.ny = (int)img->dims[1]; g.nzb = (int)img->dims[2];
  g.W = (g.nx + 63) / 64;
  g.lastpos = (g.nx - 1) & 63;
  g.wShift = g.yShift = -1;
  for (int b = 0; b < 31; b++) {
    if (g.W == (1 << b)) g.wShift = b;
    if (g.ny == (1 << b)) g.yShift = b;
  }
  g.gnz = g.nzb; g.zglob0 = 0; g.oz0 = 0; g.oz1 = g.nzb;
  g.cmapLinear = t.cmap_linear;
  return g;
}

// ---- workspace sizes: the bytes of every device buffer, reserved by count_prepare and emit_points_phase at their points of
// an extraction and by cuberille_warm_up ahead of one.  A required buffer that cannot be had fails the call
// (CUBERILLE_ERR_HIP); an optional one (0 bytes: not wanted) is done without.
struct CountSizes {
  size_t nwords, nseg;                                     // counted words, 64-word scan segments
  size_t bits, occ, prefix, segPre, blockTot, blockBase;   // required
  size_t flatBits, vqueue;                                 // optional
};

// (neither the padded nor the pitched sweep goes through the flat scratch stream)
CountSizes count_sizes(const Grid &g, const Tuning &t, const View &v) {
  const bool bordered = v.kind == VIEW_BORDER || (v.kind == VIEW_REGION && v.pitched);
  const size_t slice = (size_t)g.ny * g.W, nwords = (size_t)(g.oz1 - g.cz0) * slice, nblk = (nwords + COUNT_WB - 1) / COUNT_WB;
  CountSizes s;
  s.nwords = nwords; s.nseg = (nwords + 63) / 64;
  s.bits = (slice * g.nzb + slice) * sizeof(u64);   // (+ one slice past the buffer: quirk Q1's source from the rank below)
  s.occ = sizeof(Totals) + (size_t)g.nzb * sizeof(u32);   // the totals and the per-slice occupancy: one memset zeroes both
  s.prefix = (nwords + 4) * sizeof(u32);            // (+ the tail of a 16-byte read at the last words: locate_word_wave)
  s.segPre = s.nseg * sizeof(u64);
  s.blockTot = (nblk + 2 * (nblk / 8192 + 1)) * sizeof(u64);   // (+ the sums of its chunks of 8192: k_block_partial)
  s.blockBase = nblk * 2 * sizeof(u64);
  s.flatBits = g.nx % 64 != 0 && !bordered ? (slice * g.nzb + 32) * sizeof(u64) : 0;   // ragged rows: one flat stream, then rows
  s.vqueue = nwords < 0xffffffffULL && !t.no_vqueue ? nwords * sizeof(u32) : 0;
  return s;
}

// The dense corner -> vertex map: 4 B per lattice corner 0..nx, 0..ny, 0..nzb + 1 (the last plane also takes the handed-over
// one), in bricks or row-major (Tuning::cmap_linear).  Optional.
size_t cmap_bytes(const Grid &g, const Tuning &t) {
  if (t.no_cmap) return 0;
  return g.cmapLinear ? (size_t)(g.nx + 1) * (g.ny + 1) * (g.nzb + 2) * sizeof(u32)
                      : (((size_t)g.nx + 4) >> 2) * (((size_t)g.ny + 4) >> 2) * (((size_t)g.nzb + 3) >> 1) * 32 * sizeof(u32);
}

// The emit's buffers for nV points (ghost + owned) with room behind them for the rank below's plane of planeCorners (quirk Q1
// across slabs), nQ quads of totQ counted ones.  `cover`: what the next extraction on the context asks for when it launches
// blindly from these counts (cuberille_step_begin: + 25 %), taken where a buffer has to grow anyway (dyn: they are that).
struct Want { size_t bytes, cover; };
struct EmitSizes {
  Want rows[N_ROWS];                  // kRows: points and cells required; an attribute's while it is on and the mesh has what it hangs on
  Want compScan;                      // cuberille_set_components: the numbering's scan row (the forest is sized as the point labels)
  Want headV, headQ;                  // optional (4 B per 64 outputs)
  size_t cmap, escCap;                // optional; THIN_HALO: entries of the escape list (required there)
};

// on: the attributes as the count found them; pixel: the size of a pixel
EmitSizes emit_sizes(const Grid &g, const Tuning &t, bool triangles, bool dyn, u64 nV, u64 totQ, u64 nQ, size_t planeCorners,
                     size_t nwords, const bool on[N_ATTRS], size_t pixel) {
  const u64 nextV = dyn ? nV : nV + nV / 4 + 4096, nextQ = dyn ? nQ : totQ + totQ / 4 + 4096;
  const int nv = triangles ? 3 : 4, perQuad = triangles ? 2 : 1;     // (a quad is one cell or two)
  const size_t quad = (size_t)perQuad * nv * sizeof(u64);
  const bool heads = nwords < 0xffffffffULL && !t.no_heads;
  EmitSizes s;
  s.rows[ROW_POINTS] = {(size_t)(nV + planeCorners ? nV + planeCorners : 1) * 3 * sizeof(float), (size_t)(nextV + planeCorners) * 3 * sizeof(float)};
  s.rows[ROW_CELLS] = {(size_t)(nQ ? nQ : 1) * quad, (size_t)nextQ * quad};
  // the attributes' rows (a whole volume: no plane, no ghosts): the point and cell figures of `points` and `cells`, K <= points
  const u64 n[N_PERS] = {nV, nQ * perQuad, nV}, next[N_PERS] = {nextV, nextQ * perQuad, nextV};
  for (int r = ROW_CELLS + 1; r < N_ROWS; r++) {
    const bool wanted = on[kRows[r].attr] && n[kAttrOf[kRows[r].attr]];
    s.rows[r] = wanted ? Want{row_reserve_bytes(r, n, nv, pixel), (size_t)next[kRows[r].per] * kRows[r].elem(nv, pixel)} : Want{0, 0};
  }
  s.compScan = on[ATTR_COMPONENTS] ? Want{comp_scan_bytes(nV), comp_scan_bytes(nextV)} : Want{0, 0};   // (K's slot also for an empty mesh)
  s.headV = heads ? Want{(size_t)(nV / 64 + 2) * sizeof(u32), (size_t)(nextV / 64 + 2) * sizeof(u32)} : Want{0, 0};
  s.headQ = heads ? Want{(size_t)(totQ / 64 + 2) * sizeof(u32), (size_t)(nextQ / 64 + 2) * sizeof(u32)} : Want{0, 0};
  s.cmap = nV < 0xffffffffULL ? cmap_bytes(g, t) : 0;   // (more than 2^32 vertices: the cell kernel recomputes ids instead)
  s.escCap = nV < ESCAPE_LIST_CAP ? (size_t)nV + 1 : (size_t)ESCAPE_LIST_CAP;
  return s;
}

// The point scalars' row of an emit of nV points, beside EmitSizes::rows: 8 bytes per point, nothing for an empty mesh, and
// the cover of the points' own row (dyn, the blind launch of cuberille_extract_device: nV is that cover already)
Want point_scalars_want(u64 nV, bool dyn = false) {
  return nV ? Want{point_scalars_bytes(nV), point_scalars_bytes(dyn ? nV : nV + nV / 4 + 4096)} : Want{0, 0};
}

// An optional buffer: its pointer, or null when it is not wanted or cannot be had
void *optional(DevBuf &b, size_t bytes, size_t cover = 0) {
  if (bytes && b.reserve_covering(bytes, cover) == hipSuccess) return b.p;
  (void)hipGetLastError();
  return nullptr;
}

// cuberille_keep_components let the mesh's rows change places with spare rows sized by the kept counts.  Once that mesh is gone,
// the larger buffer of each pair is the one the extraction was sized for: back in its place, nothing is reserved again.  (The
// normals' and the cell pixels' only while their setting is on: off, its setter released both partners.)  Touches no device.
void rows_home(cuberille_ctx *c) {
  for (int r = 0; r < N_ROWS; r++) {
    const int a = kRows[r].attr;
    if (a != ATTR_NONE && a != ATTR_COMPONENTS && !c->attr[a].on) continue;
    if (c->rows[r].spare.cap > c->rows[r].row.cap) std::swap(c->rows[r].row, c->rows[r].spare);
  }
  if (c->ps.on && c->ps.rows.spare.cap > c->ps.rows.row.cap) std::swap(c->ps.rows.row, c->ps.rows.spare);   // (off: left alone)
}

// First half of a count: layout, parameters, workspace, zeroed state.  The caller then thresholds the slices
// (all at once, or z-range by z-range as they arrive) and calls count_finish.
// view: what resolve_view made of the context's settings for this image and route.
int count_prepare(cuberille_ctx *c, const cuberille_image_desc *img, const void *dev_voxels, const cuberille_params *prm,
                  const cuberille_slab *slab, const View &view) {
  c->counted = false;
  c->pointsEmitted = false;
  c->haveMesh = false;
  for (auto &a : c->attr) a.have = false;
  c->ps.have = false;
  c->hostMeshValid = false;
  c->stepMode = 0;
  c->voxelHaloEvent = nullptr;
  c->aliasBelowBuffer = false;
  c->aliasMustResolve = false;
  c->aliasZ = -1;
  rows_home(c);                              // (the mesh is gone now)
  HIP_TRY(c, hipSetDevice(c->device));

  // ---- layout -----------------------------------------------------------------------------
  const cuberille_image_desc framed = framed_desc(view, img);
  Grid g = whole_grid(&framed, c->tune);
  Geo geo{};
  Params p{};
  resolve(&framed, prm, geo, p);
  if (c->holdGradient && prm->step_length < 0.0) {
    // cuberille_hold_gradient stands for one filter OBJECT: m_ProjectVertexStepLength is replaced by its default once, at the
    // first Update(), from THAT input's spacing, and stays (txx:82-85) -- like the gradient image, the default step of every
    // later extraction is the first one's
    if (c->heldStep < 0.0) c->heldStep = p.step;
    p.step = c->heldStep;
  }
  const bool whole = whole_volume(slab);
  if (!whole) {
    if (slab->global_nz < 1 || slab->z_begin < 0 || slab->z_begin + g.nzb > slab->global_nz ||
        slab->own_z0 < slab->z_begin || slab->own_z1 > slab->z_begin + g.nzb || slab->own_z0 >= slab->own_z1)
      return fail(c, CUBERILLE_ERR_ARGUMENT, "slab ranges are inconsistent with the buffer");
    const char *why = "";                    // (the optional outputs against the slab alone: validate saw to the parameters)
    if (const int rc = attrs_offered(c, nullptr, ROUTE_SLAB, slab, g.nzb, &why)) return fail(c, rc, why);
    // the owned range needs 2 slices below (ids of corners created one slice down depend on the
    // slice below that) and 1 above; with the projection on, as far as a walk can reach (both unless the
    // volume ends there)
    // (a THIN_HALO slab promises the topology's slices only; walks that want more are put aside, not clamped)
    if (p.project && p.gradVariant != CUBERILLE_GRADIENT_CENTRAL)
      return fail(c, CUBERILLE_ERR_ARGUMENT, "the recursive-Gaussian gradient filters whole lines of the volume: not offered on slabs");
    if (p.project && c->holdGradient)
      return fail(c, CUBERILLE_ERR_ARGUMENT, "a held gradient image (cuberille_hold_gradient) belongs to a whole volume: not offered on slabs");
    if (p.project && c->interp == CUBERILLE_INTERP_BSPLINE)
      return fail(c, CUBERILLE_ERR_ARGUMENT, "the B-spline prefilter filters whole lines of the volume: not offered on slabs");
    const bool thin = (slab->flags & CUBERILLE_SLAB_THIN_HALO) != 0;
    if (thin && p.project && p.variant != CUBERILLE_PROJECT_DEFAULT)
      return fail(c, CUBERILLE_ERR_ARGUMENT, "a THIN_HALO slab is only offered with the default projection branch");
    long long halo = thin ? 0 : projection_reach(geo, p);
    const long long lo = halo > 2 ? halo : 2, hi = halo > 1 ? halo : 1;
    const long long needLo = slab->own_z0 >= lo ? slab->own_z0 - lo : 0;
    const long long needHi = slab->own_z1 + hi < slab->global_nz ? slab->own_z1 + hi : slab->global_nz;
    if (slab->z_begin > needLo || slab->z_begin + g.nzb < needHi) {
      char msg[256];
      snprintf(msg, sizeof msg, "slab buffer must hold %lld halo slices below and %lld above the owned range for these "
               "parameters (cuberille_required_halo); it holds %lld and %lld", lo, hi,
               (long long)(slab->own_z0 - slab->z_begin), (long long)(slab->z_begin + g.nzb - slab->own_z1));
      return fail(c, CUBERILLE_ERR_HALO, msg);
    }
    g.gnz = slab->global_nz; g.zglob0 = slab->z_begin;
    g.oz0 = (int)(slab->own_z0 - slab->z_begin);
    g.oz1 = (int)(slab->own_z1 - slab->z_begin);
  }
  g.cz0 = g.oz0 > 0 ? g.oz0 - 1 : 0;
  const CountSizes sz = count_sizes(g, c->tune, view);
  if (sz.nseg > 0x7fffffffULL) return fail(c, CUBERILLE_ERR_LIMIT, "volume too large for one device scan");

  // ---- workspace ----------------------------------------------------------------------------------
  HIP_TRY(c, c->bits.reserve(sz.bits));
  c->slabMode = !whole;
  c->thinHalo = !whole && (slab->flags & CUBERILLE_SLAB_THIN_HALO) != 0 && p.project;
  c->pointsStartedEarly = false;
  c->escapeChecked = false;
  c->extIds = nullptr;
  c->extPts = nullptr;
  static_assert(sizeof(Totals) % 16 == 0, "the occupancy words follow the totals");
  HIP_TRY(c, c->occ.reserve(sz.occ));
  HIP_TRY(c, c->prefix.reserve(sz.prefix));
  HIP_TRY(c, c->segPre.reserve(sz.segPre));
  HIP_TRY(c, c->blockTot.reserve(sz.blockTot));
  HIP_TRY(c, c->blockBase.reserve(sz.blockBase));
  Workspace w{};
  w.flatBits = (u64 *)optional(c->flatBits, sz.flatBits);
  w.vqueue = (u32 *)optional(c->vqueue, sz.vqueue);
  w.vox = dev_voxels;
  w.view = view;
  if (view.kind == VIEW_REGION)   // the sweep and the walk start at the box's first voxel and step by the view's pitches; nothing else reads voxels
    w.vox = (const char *)dev_voxels + (size_t)(view.start[0] + view.start[1] * view.rowPitch + view.start[2] * view.slicePitch) * pixel_size(img->pixel_type);
  w.bits = (u64 *)c->bits.p; w.sliceOcc = (u32 *)((char *)c->occ.p + sizeof(Totals));
  w.prefix = (u32 *)c->prefix.p;
  w.segPre = (u64 *)c->segPre.p; w.blockTot = (u64 *)c->blockTot.p; w.blockBase = (u64 *)c->blockBase.p;
  w.totals = (Totals *)c->occ.p;

  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemsetAsync(w.totals, 0, sz.occ, s));
  c->stagesTimed = c->tune.stage_timing != 0;
  c->lightTiming = !c->stagesTimed && (u64)g.nx * (u64)g.ny * (u64)g.nzb <= (4ull << 20);
  HIP_TRY(c, mark(c, PASS_BEGIN));
  c->g = g; c->geo = geo; c->prm = p; c->pixel_type = img->pixel_type; c->w = w;
  c->countBsBits = (p.project && c->interp == CUBERILLE_INTERP_BSPLINE) ? c->bsBits : 0;
  for (auto &a : c->attr) a.counting = a.on;
  c->ps.counting = c->ps.on;
  c->nwords = sz.nwords; c->nseg = sz.nseg;
  return CUBERILLE_OK;
}

// Second half: count + scan of the thresholded volume (launches only).
int count_launch(cuberille_ctx *c, const Gate &gate) {
  hipStream_t s = c->stream;
  HIP_TRY(c, mark(c, CLASSIFY_END));
  HIP_TRY(c, launch_occupancy(c->pixel_type, c->w, c->g, c->tune, s));
  // (the LDS-tiled form pays where most words carry surface -- 2048^3 noise -- and costs where few do: it stages every
  //  row, a sparse block's untiled form skips whole words; the previous extraction's density decides)
  int tiled = c->tune.count_variant >= 0 ? c->tune.count_variant : (c->haveHistory && c->histDense ? 3 : 0);
  // A launch whose blocks are all resident at once is a block's latency, whatever the field: eight dependent trips to memory per
  // thread for the faces (2600 cycles each, profiles/microbench/r5_count_phase_stamps.log) and two or three more for the corner
  // logic from memory; the LDS tile (one block per workgroup) makes that one coalesced copy -- 512^3 sphere 0.0352 -> 0.0309 ms,
  // 512^3 Marschner-Lobb 0.0466 -> 0.0388; with several rounds of blocks (768^3: 3456) the form that skips empty words wins again.
  if (c->tune.count_variant < 0 && tiled == 0 && (c->nwords + COUNT_WB - 1) / COUNT_WB <= 1280 && (c->nwords + COUNT_WB - 1) / COUNT_WB > 64)
    tiled = 2;
  if (c->tune.count_variant < 0 && !c->haveHistory && c->nwords >= (1u << 22) && c->g.wShift >= 0) {
    // no previous extraction to go by (round-4 review: a one-shot caller of a dense field paid 2.3 ms for a 1.2 ms count):
    // a sample of THIS volume's bit volume picks the form -- one small launch and one more wait, on a context's first
    // extraction only, which waits for its counts anyway.  (Totals::iters carries the sample: the walk, which counts its
    // passes there, is a long way off; zeroed again behind the read.)
    u64 *slot = &c->w.totals->iters;
    HIP_TRY(c, launch_density_probe(c->w, c->g, c->nwords, slot, s));
    HIP_TRY(c, hipMemcpyAsync(&c->hostTotals->iters, slot, sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemsetAsync(slot, 0, sizeof(u64), s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const u64 v = c->hostTotals->iters;
    const u64 mixed = v & 0xffffffffull, sampled = v >> 32;
    if (sampled && mixed * 4 >= sampled) tiled = 3;
  }
  HIP_TRY(c, launch_count(c->w, c->g, c->nwords, c->prm.q1, gate, tiled, c->tune.count_no_fold, s));
  HIP_TRY(c, mark(c, PASS_END));
  return CUBERILLE_OK;
}

// the totals (and a slab's per-slice occupancy) on their way to pinned memory
int totals_to_host(cuberille_ctx *c) {
  hipStream_t s = c->stream;
  const Grid &g = c->g;
  HIP_TRY(c, hipMemcpyAsync(c->hostTotals, c->w.totals, sizeof(Totals), hipMemcpyDeviceToHost, s));
  if (c->slabMode) {
    // the slab status the multi-GPU driver asks for next rides in the same synchronisation
    if (c->hostOccCap < (size_t)g.nzb) {
      if (c->hostOcc) (void)hipHostFree(c->hostOcc);
      c->hostOcc = nullptr;
      c->hostOccCap = 0;
      HIP_TRY(c, hipHostMalloc((void **)&c->hostOcc, (size_t)g.nzb * sizeof(uint32_t), hipHostMallocDefault));
      c->hostOccCap = (size_t)g.nzb;
    }
    HIP_TRY(c, hipMemcpyAsync(c->hostOcc, c->w.sliceOcc, (size_t)g.nzb * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  return CUBERILLE_OK;
}

// ... and, once the stream has been waited for, taken over as the state of a finished count
void adopt_totals(cuberille_ctx *c, uint64_t *n_points, uint64_t *n_cells) {
  const Grid &g = c->g;
  c->tot = *c->hostTotals;
  // quirk Q1 reaching below this slab: certain when the source slice is in the halo (the emit then insists on
  // cuberille_recount), possible when the search ran off the buffer's bottom (the ranks below know)
  c->aliasMustResolve = (c->tot.err & ERRF_ALIAS_UNKNOWN) != 0;
  c->aliasBelowBuffer = (c->tot.err & (ERRF_ALIAS_BELOW_BUFFER | ERRF_ALIAS_UNKNOWN)) != 0;
  // the slice it concerns: only the FIRST occupied slice of the counted range can have its source outside of it
  if (c->slabMode && c->aliasZ < 0 && c->aliasBelowBuffer)
    for (int z = g.cz0; z < g.oz1; z++)
      if (c->hostOcc[(size_t)z]) { c->aliasZ = z; break; }
  c->counted = true;
  std::memset(&c->res, 0, sizeof(c->res));
  c->res.n_points = c->tot.totV - c->tot.V0;
  c->res.n_cells = (c->tot.totQ - c->tot.Q0) * (c->prm.triangles ? 2 : 1);
  c->res.verts_per_cell = c->prm.triangles ? 3 : 4;
  if (n_points) *n_points = c->res.n_points;
  if (n_cells) *n_cells = c->res.n_cells;
}

int classify_slab(cuberille_ctx *c, const cuberille_image_desc *img, const cuberille_slab *slab);

int count_finish(cuberille_ctx *c, uint64_t *n_points, uint64_t *n_cells) {
  int rc = count_launch(c, Gate{});
  if (rc) return rc;
  rc = totals_to_host(c);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  adopt_totals(c, n_points, n_cells);
  return CUBERILLE_OK;
}

}  // namespace

extern "C" {

int cuberille_required_halo(const cuberille_image_desc *img, const cuberille_params *prm, int64_t *below, int64_t *above) {
  if (!img || !prm) return CUBERILLE_ERR_ARGUMENT;
  for (int i = 0; i < 3; i++) if (!(img->spacing[i] > 0.0)) return CUBERILLE_ERR_ARGUMENT;
  Geo geo{};
  Params p{};
  resolve(img, prm, geo, p);
  const long long halo = projection_reach(geo, p);
  if (below) *below = halo > 2 ? halo : 2;
  if (above) *above = halo > 1 ? halo : 1;
  return CUBERILLE_OK;
}

int cuberille_minimum_halo(const cuberille_image_desc *img, const cuberille_params *prm, int64_t *below, int64_t *above) {
  if (!img || !prm) return CUBERILLE_ERR_ARGUMENT;
  for (int i = 0; i < 3; i++) if (!(img->spacing[i] > 0.0)) return CUBERILLE_ERR_ARGUMENT;
  Geo geo{};
  Params p{};
  resolve(img, prm, geo, p);
  long long lo = 2, hi = 1;                      // the topology: ghost slice + the one under it; one slice above
  if (p.project) {
    // a vertex starts at index-space z = cz + oz, oz = -(row z of PhysicalPointToIndex) . spacing / 2 (txx:266-270: the
    // half-spacing shift is taken per PHYSICAL axis; -1/2 for an axis-aligned image); its cell floor(cz + oz) reads
    // slices floor - 1 .. floor + 2 (gradient ring).  Vertices that matter sit on planes own_z0 .. own_z1.
    double oz = 0.0;
    for (int k = 0; k < 3; k++) oz -= geo.p2i[6 + k] * (geo.spacing[k] / 2.0);
    // (compared in double and capped like projection_reach: under a spacing of (1e12, 1, 1e-12) and a tilted direction oz is
    //  beyond 2^63, and a conversion of that to an integer is not defined -- it used to hand out a negative halo)
    const double b = 1.0 - std::floor(oz - 1e-6), a = std::floor(oz + 1e-6) + 3.0;
    if (!(b <= (double)lo)) lo = b < 1e9 ? (long long)b : 1000000000LL;
    if (!(a <= (double)hi)) hi = a < 1e9 ? (long long)a : 1000000000LL;
  }
  if (below) *below = lo;
  if (above) *above = hi;
  return CUBERILLE_OK;
}

int cuberille_count(cuberille_ctx *c, const cuberille_image_desc *img, const void *dev_voxels,
                    const cuberille_params *prm, const cuberille_slab *slab, uint64_t *n_points, uint64_t *n_cells) {
  int rc = validate(c, img, dev_voxels, prm);
  if (rc) return rc;
  View view;
  rc = view_of(c, img, prm, whole_volume(slab) ? ROUTE_DEVICE : ROUTE_SLAB, &view);
  if (rc) return rc;
  rc = count_prepare(c, img, dev_voxels, prm, slab, view);
  if (rc) return rc;
  rc = classify_slab(c, img, slab);
  if (rc) return rc;
  return count_finish(c, n_points, n_cells);
}

}  // extern "C"

namespace {

// threshold the buffer of a prepared count: at once, or the owned slices now and the halo slices behind the caller's event
int classify_slab(cuberille_ctx *c, const cuberille_image_desc *img, const cuberille_slab *slab) {
  const Grid &g = c->g;
  hipStream_t s = c->stream;
  if (slab && slab->voxels_ready_event) HIP_TRY(c, hipStreamWaitEvent(s, (hipEvent_t)slab->voxels_ready_event, 0));
  if (slab && slab->halo_ready_event && (g.oz0 > 0 || g.oz1 < g.nzb)) {
    // the caller's halo exchange is still in flight: threshold the owned slices now, the halo
    // slices once the event it recorded behind the exchange has fired
    HIP_TRY(c, launch_classify(img->pixel_type, c->w, g, c->prm, g.oz0, g.oz1, c->tune, s));
    HIP_TRY(c, hipStreamWaitEvent(s, (hipEvent_t)slab->halo_ready_event, 0));
    HIP_TRY(c, launch_classify(img->pixel_type, c->w, g, c->prm, 0, g.oz0, c->tune, s));
    HIP_TRY(c, launch_classify(img->pixel_type, c->w, g, c->prm, g.oz1, g.nzb, c->tune, s));
  } else {
    // (with a border the grid is two slices taller than the buffer the sweep reads)
    HIP_TRY(c, launch_classify(img->pixel_type, c->w, g, c->prm, 0, g.nzb - (c->w.view.kind == VIEW_BORDER ? 2 : 0), c->tune, s));
  }
  return CUBERILLE_OK;
}

}  // namespace

extern "C" {

int cuberille_recount(cuberille_ctx *c, const void *dev_source_bits, uint64_t *n_points, uint64_t *n_cells) {
  if (!c || !dev_source_bits) return CUBERILLE_ERR_ARGUMENT;
  if (!c->counted || !c->slabMode)
    return fail(c, CUBERILLE_ERR_STATE, "cuberille_recount follows a successful cuberille_count on a slab");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t sliceWords = (size_t)c->g.ny * c->g.W;
  // the source slice goes one past the buffer's last slice; the count then finds it where alias_of points
  HIP_TRY(c, hipMemcpyAsync((u64 *)c->bits.p + sliceWords * (size_t)c->g.nzb, dev_source_bits, sliceWords * sizeof(u64),
                            hipMemcpyDeviceToDevice, s));
  c->g.extAlias = 1;
  c->counted = false;
  c->pointsEmitted = false;                  // the counts change: whatever cuberille_emit_points started is void
  c->pointsStartedEarly = false;
  c->escapeChecked = false;
  HIP_TRY(c, hipMemsetAsync(c->w.totals, 0, sizeof(Totals), s));
  HIP_TRY(c, mark(c, PASS_BEGIN));           // ms_pass of a recounted slab: this count alone, not the host time since the first
  return count_finish(c, n_points, n_cells);
}

int cuberille_slice_bits_device(cuberille_ctx *c, int64_t z_global, const uint64_t **dev_words, size_t *n_words) {
  if (!c || !dev_words || !n_words) return CUBERILLE_ERR_ARGUMENT;
  if (!c->counted && !c->haveMesh) return fail(c, CUBERILLE_ERR_STATE, "no classified volume on this context");
  const long long z = z_global - c->g.zglob0;
  if (z < 0 || z >= c->g.nzb) return fail(c, CUBERILLE_ERR_ARGUMENT, "slice outside the buffer");
  *n_words = (size_t)c->g.ny * c->g.W;
  *dev_words = (const uint64_t *)c->bits.p + *n_words * (size_t)z;
  return CUBERILLE_OK;
}

int cuberille_alias_plane_device(cuberille_ctx *c, int64_t z_global, uint64_t *dev_ids, float *dev_points) {
  if (!c || !dev_ids || !dev_points) return CUBERILLE_ERR_ARGUMENT;
  if (!c->haveMesh) return fail(c, CUBERILLE_ERR_STATE, "no mesh: the plane is built from the last emit");
  const long long z = z_global - c->g.zglob0;
  if (z < c->g.oz0 || z >= c->g.oz1) return fail(c, CUBERILLE_ERR_ARGUMENT, "slice outside the owned range");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, launch_alias_plane(c->w, c->g, (int)z, c->pointOffset, (u64 *)dev_ids, dev_points, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CUBERILLE_OK;
}

int cuberille_set_alias_plane(cuberille_ctx *c, const uint64_t *dev_ids, const float *dev_points) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (!c->counted || !c->g.extAlias)
    return fail(c, CUBERILLE_ERR_STATE, "cuberille_set_alias_plane follows cuberille_recount and precedes cuberille_emit");
  c->extIds = (const u64 *)dev_ids;
  c->extPts = dev_points;
  return CUBERILLE_OK;
}

}  // extern "C"

namespace {

// The part of the emit that needs no id offsets: buffers, head tables, vertex scatter, projection.  Runs once per count
// (cuberille_emit_points may have started it already, while the caller was gathering the counts of the other ranks).
// dyn (cuberille_step_begin): buffers and launches are sized for the cover values, the kernels read the real counts
// from the device and run only when they fit (Totals::go).
int emit_points_phase(cuberille_ctx *c, bool ahead, bool dyn = false, u64 coverV = 0, u64 coverQ = 0, u32 coverVW = 0) {
  if (c->pointsEmitted) return CUBERILLE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const u64 nV = dyn ? coverV : c->tot.totV;                 // ghost + owned
  const u64 nGhost = dyn ? 0 : c->tot.V0;
  const u64 totQ = dyn ? coverQ : c->tot.totQ;
  const u64 nQ = dyn ? coverQ : c->tot.totQ - c->tot.Q0;
  const u32 nVW = dyn ? coverVW : c->tot.nVertexWords;
  // room behind this rank's points for the positions of a plane of the rank below's vertices (quirk Q1 across slabs)
  const size_t planeCorners = (c->slabMode || c->g.extAlias) ? (size_t)(c->g.nx + 1) * (c->g.ny + 1) : 0;
  bool counting[N_ATTRS];
  for (int a = 0; a < N_ATTRS; a++) counting[a] = c->attr[a].counting;
  const EmitSizes sz = emit_sizes(c->g, c->tune, c->prm.triangles, dyn, nV, totQ, nQ, planeCorners, c->nwords, counting,
                                  pixel_size(c->pixel_type));
  // (cuberille_set_components: uint32 labels, like the corner map's entries)
  if (c->attr[ATTR_COMPONENTS].counting && nV >= 0xffffffffULL)
    return fail(c, CUBERILLE_ERR_ARGUMENT, "components (cuberille_set_components) are 32-bit labels: not offered with 2^32 points or more");
  for (int r = 0; r < N_ROWS; r++) {
    const Want &want = sz.rows[r];
    if (!want.bytes) continue;
    if (r == ROW_COMP_POINT)   // (the components' forest: scratch, ahead of the point labels it turns into and sized as they are)
      HIP_TRY(c, c->compParent.reserve_covering(want.bytes, want.cover));
    HIP_TRY(c, c->row(r).reserve_covering(want.bytes, want.cover));
  }
  // (the point scalars' row, beside the table: 8 bytes per point, none for an empty mesh)
  const Want scalarsWant = c->ps.counting ? point_scalars_want(nV, dyn) : Want{0, 0};
  const bool scalars = scalarsWant.bytes != 0;
  if (scalars) HIP_TRY(c, c->ps.rows.row.reserve_covering(scalarsWant.bytes, scalarsWant.cover));
  if (sz.compScan.bytes) {
    HIP_TRY(c, c->compScan.reserve_covering(sz.compScan.bytes, sz.compScan.cover));
    if (!c->hostK) HIP_TRY(c, hipHostMalloc((void **)&c->hostK, sizeof(u64), hipHostMallocDefault));
  }
  Workspace &w = c->w;
  w.points = (float *)c->row(ROW_POINTS).p;
  w.cells = (u64 *)c->row(ROW_CELLS).p;
  // without the corner map the cell kernel recomputes ids, without the head tables the waves search their outputs' words
  w.cmap = (u32 *)optional(c->cmap, sz.cmap);
  w.headQ = (u32 *)optional(c->headQ, sz.headQ.bytes, sz.headQ.cover);
  w.headV = w.vqueue ? nullptr : (u32 *)optional(c->headV, sz.headV.bytes, sz.headV.cover);
  // THIN_HALO: room for the vertices whose walk leaves the buffer (more than these: the step is redone with the deep halo)
  w.escList = nullptr;
  w.escCap = 0;
  if (c->thinHalo) {
    HIP_TRY(c, c->escList.reserve(sz.escCap * sizeof(u32)));
    w.escList = (u32 *)c->escList.p;
    w.escCap = (u32)sz.escCap;
  }
  // (the blind form needs every scratch table: the fallbacks without them size their launches from the counts)
  if (dyn && (!w.cmap || !w.headQ || !w.vqueue || c->tune.points_variant != 3))
    return fail(c, CUBERILLE_ERR_STATE, "internal: blind launch without the scratch tables");
  hipStream_t s = c->stream;
  HIP_TRY(c, mark(c, POINTS_BEGIN));
  HIP_TRY(c, launch_heads(w, c->g, nV, totQ, dyn ? 1 : 0, s));
  HIP_TRY(c, launch_emit_points(w, c->g, c->geo, c->prm.q1, nV, nVW, c->tune, dyn ? 1 : 0, s));
  HIP_TRY(c, mark(c, POINTS_END));
  w.gradImg = nullptr;
  if (c->prm.project && c->prm.gradVariant == CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN && nV) {
    // the whole-image gradient pre-pass of txx:478-498 in its recursive-Gaussian form (the shipped central differences
    // are evaluated on the fly inside the walk and never materialised)
    const size_t nvox = (size_t)c->g.nx * c->g.ny * c->g.nzb;
    HIP_TRY(c, c->gradImg.reserve(nvox * 3 * sizeof(double)));
    HIP_TRY(c, c->rgScratch.reserve(nvox * sizeof(double)));
    HIP_TRY(c, c->rgA.reserve(nvox * sizeof(float)));
    HIP_TRY(c, c->rgB.reserve(nvox * sizeof(float)));
    w.gradImg = (double *)c->gradImg.p; w.rgScratch = (double *)c->rgScratch.p;
    w.rgA = (float *)c->rgA.p; w.rgB = (float *)c->rgB.p;
    double sigma = c->geo.spacing[0];                        // txx:489: m_MaxSpacing * 1.0
    for (int i = 1; i < 3; i++) if (c->geo.spacing[i] > sigma) sigma = c->geo.spacing[i];
    double coef[3][2][20];
    for (int ax = 0; ax < 3; ax++) {
      deriche_setup(sigma, c->geo.spacing[ax], 1, coef[ax][0]);
      deriche_setup(sigma, c->geo.spacing[ax], 0, coef[ax][1]);
    }
    HIP_TRY(c, launch_recursive_gaussian(c->pixel_type, w, c->g, c->geo, coef, s));
  }
  if (c->prm.project) {
    // (walks that end after two or three passes -- a noise field -- leave the kernel bound by its gathers, which a refill
    //  issues for the few lanes it fills: such fields refill only empty waves.  Scheduling only: results never depend on it.)
    Tuning tn = c->tune;
    // (long walks refill at 32 idle lanes: 1.161-1.166 ms against 1.178-1.192 at 16 on the headline field, three boxes, round 5;
    //  24 and 40 are no better, 48 loses 8 %)
    // (... and at 24 below 8 M vertices: 512^3 Marschner-Lobb 0.387 against 0.398 / 0.403 ms at 16 / 32, 768^3 0.702 against
    //  0.717 / 0.718)
    if (tn.proj_short < 0) tn.proj_short = c->haveHistory && c->histShortWalks ? 1 : 0;
    if (tn.proj_refill <= 0) tn.proj_refill = tn.proj_short ? 64 : (nV >= 8000000ull ? 32 : 24);
    if (c->voxelHaloEvent) {                 // the first reader of the halo's voxels
      HIP_TRY(c, hipStreamWaitEvent(s, c->voxelHaloEvent, 0));
      c->voxelHaloEvent = nullptr;
    }
    w.held = c->holdGradient && c->held.img ? &c->held : nullptr;
    if (c->countBsBits && nV) {
      // cuberille_set_interpolator(CUBERILLE_INTERP_BSPLINE): the coefficient image of the whole volume, then the walk reading it
      // (a whole volume, the default branch, the central gradient: count_prepare and validate saw to that)
      const size_t nvox = (size_t)c->g.nx * c->g.ny * c->g.nzb;
      c->bsValidBits = 0;
      HIP_TRY(c, c->bsCoef.reserve(nvox * (size_t)(c->countBsBits / 8)));
      double *scratch = nullptr;
      if (c->countBsBits == 32) {
        HIP_TRY(c, c->bsScratch.reserve(nvox * sizeof(double)));
        scratch = (double *)c->bsScratch.p;
      }
      const BsAxis ax[3] = {bspline_axis(c->g.nx), bspline_axis(c->g.ny), bspline_axis(c->g.nzb)};
      HIP_TRY(c, launch_bspline_prefilter(c->pixel_type, w.vox, c->g, ax, c->bsCoef.p, c->countBsBits, scratch, s));
      HIP_TRY(c, launch_project_bspline(c->pixel_type, w, c->g, c->geo, c->prm, nV, c->bsCoef.p, c->countBsBits, s));
      c->bsValidBits = c->countBsBits;
      c->bsDims[0] = c->g.nx; c->bsDims[1] = c->g.ny; c->bsDims[2] = c->g.nzb;
    } else {
      HIP_TRY(c, launch_project(c->pixel_type, w, c->g, c->geo, c->prm, nV, nGhost, tn, c->thinHalo ? 1 : 0, dyn ? 1 : 0, s));
    }
    if (c->holdGradient && !c->held.img) {
      // quirk Q3 on request: this is the context's first projecting extraction -- ComputeGradientImage() of txx:478-498
      // runs (the walk above evaluated the same taps on the fly) and its image stays for every extraction to come
      const size_t nvox = (size_t)c->g.nx * c->g.ny * c->g.nzb;
      HIP_TRY(c, c->heldGrad.reserve(nvox * 3 * sizeof(float)));
      HIP_TRY(c, launch_gradient_image(c->pixel_type, w, c->g, c->geo, (float *)c->heldGrad.p, s));
      c->held.img = (const float *)c->heldGrad.p;
      c->held.geo = c->geo;
      c->held.n[0] = c->g.nx; c->held.n[1] = c->g.ny; c->held.n[2] = c->g.nzb;
    }
  }
  // cuberille_set_point_normals: the points are final -- behind the walk, or behind the vertex scatter with the projection off --
  // and one more pass reads each of them once (with stage timing on, part of ms_project)
  if (sz.rows[ROW_NORMALS].bytes)
    HIP_TRY(c, launch_point_normals(c->pixel_type, w, c->g, c->geo, (float *)c->row(ROW_NORMALS).p, nV, dyn ? 1 : 0, s));
  // cuberille_set_point_scalars: the second image at the final points, one more pass behind that one (part of ms_project too)
  if (scalars)
    HIP_TRY(c, launch_point_scalars(c->ps.pixel_type, c->ps.vox, c->ps.n, c->ps.geo, (const float *)w.points, (double *)c->ps.rows.row.p,
                                    nV, (const Totals *)w.totals, dyn ? 1 : 0, c->ps.outside, s));
  if (ahead) c->pointsStartedEarly = true;   // the caller turns to the other ranks now: the cells come as an interval of their own
  HIP_TRY(c, mark(c, PROJECT_END));
  c->pointsEmitted = true;
  return CUBERILLE_OK;
}

// ---- timing marks: each mode records what finish_result reads, no more (an event between two kernels idles the stream for
// 8-10 us, as long as the kernels of a small volume take).  With stage timing off: light = at most 4 Mi voxels (lightTiming),
// one call = cuberille_extract_device (oneCall), default = the rest; stages = Tuning::stage_timing as it was when the count
// ran (stagesTimed).  split: the vertex phase ran ahead of the cells (pointsStartedEarly: cuberille_emit_points ahead of
// cuberille_emit, also after cuberille_recount; a step).
//   mark          recorded                                     light  one call  default  stages
//   PASS_BEGIN    count_prepare, cuberille_recount               x       x         x        x
//   CLASSIFY_END  count_launch, ahead of the count               .       .         .        x
//   PASS_END      count_launch, behind the count                 .       x         x        x
//   POINTS_BEGIN  emit_points_phase, ahead of the heads          .       .         x        x
//   POINTS_END    emit_points_phase, behind the vertex scatter   .       .         .        x
//   PROJECT_END   emit_points_phase, at its end                  .       .       split      x
//   CELLS_BEGIN   cuberille_emit, _step_end: ahead of the cells  .       .       split    split
//   END           cuberille_emit, _step_end: behind the cells    x       x         x        x
hipError_t mark(cuberille_ctx *c, Mark m) {
  const bool stages = c->stagesTimed, coarse = !c->lightTiming && !c->oneCall, split = c->pointsStartedEarly;
  const bool on[8] = {true, stages, !c->lightTiming, split && (stages || coarse), stages || coarse, stages,
                      stages || (split && coarse), true};   // (in the order of enum Mark)
  return on[m] ? hipEventRecord(c->ev[m], c->stream) : hipSuccess;
}

// After the last kernel of an extraction has completed and the totals are back in pinned memory: statistics, device times.
int finish_result(cuberille_ctx *c, cuberille_result *res) {
  c->tot.iters = c->hostTotals->iters;
  c->tot.stopSteps = c->hostTotals->stopSteps;
  c->tot.stopThr = c->hostTotals->stopThr;
  c->tot.nEscaped = c->hostTotals->nEscaped;
  c->tot.err = c->hostTotals->err;
  cuberille_result &r = c->res;
  auto ms = [c](float *out, Mark from, Mark to) { return hipEventElapsedTime(out, c->ev[from], c->ev[to]); };
  const bool split = c->pointsStartedEarly;
  r.ms_scan = 0.0f;                          // the prefix sums are part of the count stage (k_count + k_block_scan)
  if (c->stagesTimed) {
    HIP_TRY(c, ms(&r.ms_classify, PASS_BEGIN, CLASSIFY_END));
    HIP_TRY(c, ms(&r.ms_count, CLASSIFY_END, PASS_END));
    HIP_TRY(c, ms(&r.ms_emit_points, POINTS_BEGIN, POINTS_END));
    HIP_TRY(c, ms(&r.ms_project, POINTS_END, PROJECT_END));
    HIP_TRY(c, ms(&r.ms_emit_cells, split ? CELLS_BEGIN : PROJECT_END, END));
  }
  float b = 0.f, b2 = 0.f;
  if (c->lightTiming) {
    // one event pair: the whole extraction as the stream saw it (a host turn between count and emit included, where
    // the caller took one); no pass figure
    HIP_TRY(c, ms(&b, PASS_BEGIN, END));
    r.ms_pass = 0.f;
  } else if (c->oneCall && !c->stagesTimed) {
    // one call, no host turn in the middle: the pass, and everything behind it
    HIP_TRY(c, ms(&r.ms_pass, PASS_BEGIN, PASS_END));
    HIP_TRY(c, ms(&b, PASS_END, END));
  } else {
    HIP_TRY(c, ms(&r.ms_pass, PASS_BEGIN, PASS_END));
    if (split) {
      HIP_TRY(c, ms(&b, POINTS_BEGIN, PROJECT_END));
      HIP_TRY(c, ms(&b2, CELLS_BEGIN, END));
    } else {
      HIP_TRY(c, ms(&b, POINTS_BEGIN, END));
    }
  }
  r.ms_total = r.ms_pass + b + b2;           // device time: the host's turn between count and emit is in none of the intervals
  r.proj_iterations = c->tot.iters;
  r.proj_stop_steps = r.proj_stop_threshold = 0;
  if (c->prm.project) {
    r.proj_stop_steps = c->tot.stopSteps;
    // the default branch ends every walk one way or the other (txx:456-472): k_project counts only the rare way; the B-spline
    // walk counts both, and the two counts must then add up to the points
    r.proj_stop_threshold = c->prm.variant == CUBERILLE_PROJECT_DEFAULT && !c->countBsBits ? r.n_points - c->tot.stopSteps : c->tot.stopThr;
    if (c->countBsBits && r.proj_stop_threshold + r.proj_stop_steps != r.n_points)
      return fail(c, CUBERILLE_ERR_STATE, "internal: the B-spline walk's termination counts do not add up to the points");
  }
  r.n_escaped = c->tot.nEscaped;
  // what this extraction produced sizes the blind launches of the next cuberille_step_begin on this context
  c->haveHistory = true;
  c->histV = c->tot.totV; c->histQ = c->tot.totQ; c->histVW = c->tot.nVertexWords;
  c->histDense = (u64)c->tot.nVertexWords * 4 >= (u64)c->nwords;
  c->histShortWalks = c->prm.project && c->tot.iters > 0 && c->tot.iters < 4 * c->tot.totV;
  c->stepMode = 0;
  c->haveMesh = true;
  for (auto &a : c->attr) a.have = a.counting;
  c->ps.have = c->ps.counting;
  c->nComponents = c->attr[ATTR_COMPONENTS].counting && c->hostK ? *c->hostK : 0;
  c->counted = false;                        // the workspace now belongs to this mesh
  if (res) *res = r;
  return CUBERILLE_OK;
}

// The tail of the cell phase, behind launch_emit_cells and ahead of mark(END) (with stage timing on, part of ms_emit_cells): one
// more pass over the quads reads each one's voxel; the union-find over the cells, the numbering, the labels.  base: the point id
// offset; nV, nQ: points and quads, or with dyn what the launches and the rows are sized for.
int launch_cell_attrs(cuberille_ctx *c, u64 base, u64 nV, u64 nQ, bool dyn) {
  if (c->attr[ATTR_CELL_PIXELS].counting)
    HIP_TRY(c, launch_cell_pixels(c->pixel_type, c->w, c->g, c->prm.triangles, c->row(ROW_CELL_PIX).p, nQ, dyn ? 1 : 0, c->stream));
  if (c->attr[ATTR_COMPONENTS].counting)
    HIP_TRY(c, launch_components(c->w, comp_rows(c), c->prm.triangles, base, nV, nQ, dyn ? 1 : 0, c->stream));
  return CUBERILLE_OK;
}
// ... and behind mark(END): K rides with the totals, ahead of the one wait
int component_count_to_host(cuberille_ctx *c) {
  if (c->attr[ATTR_COMPONENTS].counting && c->hostK && c->compScan.p)
    HIP_TRY(c, hipMemcpyAsync(c->hostK, c->compScan.p, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  return CUBERILLE_OK;
}

int emit_preconditions(cuberille_ctx *c, const char *who) {
  if (!c->counted) return fail(c, CUBERILLE_ERR_STATE, std::string(who) + " called before a successful cuberille_count");
  if (c->aliasMustResolve)
    return fail(c, CUBERILLE_ERR_HALO,
                "an empty slice makes the reference re-use vertices created below this slab's counted range: hand the "
                "source slice over with cuberille_recount (DESIGN.md Q1)");
  return CUBERILLE_OK;
}

}  // namespace

extern "C" {

int cuberille_emit_points(cuberille_ctx *c) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  int rc = emit_preconditions(c, "cuberille_emit_points");
  if (rc) return rc;
  return emit_points_phase(c, true);
}

int cuberille_escaped_count(cuberille_ctx *c, uint64_t *n_escaped) {
  if (!c || !n_escaped) return CUBERILLE_ERR_ARGUMENT;
  if (!c->counted || !c->pointsEmitted)
    return fail(c, CUBERILLE_ERR_STATE, "cuberille_escaped_count follows cuberille_emit_points");
  *n_escaped = 0;
  if (!c->thinHalo) return CUBERILLE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(c->hostTotals, c->w.totals, sizeof(Totals), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->tot.nEscaped = c->hostTotals->nEscaped;
  c->tot.err = c->hostTotals->err;
  c->escapeChecked = true;
  *n_escaped = (c->tot.err & ERRF_ESCAPE_OVERFLOW) ? UINT64_MAX : (uint64_t)c->tot.nEscaped;
  return CUBERILLE_OK;
}

int cuberille_reproject_escaped(cuberille_ctx *c, const void *dev_voxels, int64_t z_begin, int64_t nz) {
  if (!c || !dev_voxels) return CUBERILLE_ERR_ARGUMENT;
  if (!c->counted || !c->pointsEmitted || !c->thinHalo)
    return fail(c, CUBERILLE_ERR_STATE, "cuberille_reproject_escaped follows cuberille_emit_points on a THIN_HALO slab");
  if (c->w.view.kind == VIEW_BORDER)   // (cannot happen: a slab count refuses the border -- said here so that it never becomes a bare launch error)
    return fail(c, CUBERILLE_ERR_ARGUMENT, std::string(kViewWords[VIEW_BORDER].noun) + " (" + kViewWords[VIEW_BORDER].fn + ")" +
                                               kViewWords[VIEW_BORDER].route[ROUTE_SLAB]);
  if (c->tot.err & ERRF_ESCAPE_OVERFLOW)
    return fail(c, CUBERILLE_ERR_LIMIT, "more walks left the thin halo than the escape list holds: count the slab again with "
                                        "the full halo (cuberille_required_halo)");
  // the deeper buffer must hold what a slab without the flag would have had to
  const long long reach = projection_reach(c->geo, c->prm);
  const long long lo = reach > 2 ? reach : 2, hi = reach > 1 ? reach : 1;
  const long long own0 = c->g.zglob0 + c->g.oz0, own1 = c->g.zglob0 + c->g.oz1;
  const long long needLo = own0 >= lo ? own0 - lo : 0, needHi = own1 + hi < c->g.gnz ? own1 + hi : c->g.gnz;
  if (nz < 1 || z_begin < 0 || z_begin + nz > c->g.gnz || z_begin > needLo || z_begin + nz < needHi)
    return fail(c, CUBERILLE_ERR_HALO, "the deeper buffer does not hold the halo these parameters need (cuberille_required_halo)");
  const u64 n = c->tot.nEscaped;
  if (n == 0) return CUBERILLE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  Grid deep = c->g;
  deep.nzb = (int)nz;
  deep.zglob0 = z_begin;
  Workspace w = c->w;
  w.vox = dev_voxels;
  Tuning tn = c->tune;
  if (tn.proj_refill <= 0) tn.proj_refill = 16;
  HIP_TRY(c, launch_project(c->pixel_type, w, deep, c->geo, c->prm, n, c->tot.V0, tn, 2, 0, c->stream));
  // nobody waits any more (the list's length travelled by value): the device-side counter starts over
  HIP_TRY(c, hipMemsetAsync(&c->w.totals->nEscaped, 0, sizeof(u32), c->stream));
  c->tot.nEscaped = 0;
  return CUBERILLE_OK;
}

int cuberille_emit(cuberille_ctx *c, uint64_t point_id_offset, cuberille_result *res) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  int rc = emit_preconditions(c, "cuberille_emit");
  if (rc) return rc;
  // (a recount for the ghost slice needed the source's bits only: that slice emits no cells)
  const bool needPlane = c->g.extAlias && c->aliasZ >= c->g.oz0;
  if (needPlane && (!c->extIds || !c->extPts))
    return fail(c, CUBERILLE_ERR_STATE, "cuberille_emit after cuberille_recount needs cuberille_set_alias_plane");
  c->slabMesh = point_id_offset != 0 || c->tot.V0 != 0 || part_of_a_volume(c->g);
  c->pointOffset = point_id_offset;
  rc = emit_points_phase(c, false);
  if (rc) return rc;
  if (c->thinHalo) {
    // no cell is written while a vertex waits for slices this buffer lacks (the count and the vertex phase stand: the
    // caller fetches the deeper halo, calls cuberille_reproject_escaped and comes back)
    uint64_t nEsc = c->tot.nEscaped;
    if (!c->escapeChecked && (rc = cuberille_escaped_count(c, &nEsc)) != CUBERILLE_OK) return rc;
    if (nEsc)
      return fail(c, CUBERILLE_ERR_HALO, std::to_string(nEsc) + " walks left the thin halo: cuberille_reproject_escaped "
                                         "with the deeper buffer comes before cuberille_emit");
  }
  const u64 nV = c->tot.totV;
  const u64 nQ = c->tot.totQ - c->tot.Q0;
  const size_t planeCorners = needPlane ? (size_t)(c->g.nx + 1) * (c->g.ny + 1) : 0;   // positions of the rank below's vertices
  Workspace &w = c->w;
  hipStream_t s = c->stream;
  // the vertex phase was started ahead of this call (cuberille_emit_points): the device may have idled since, waiting
  // for the host's all-gather -- the cell phase is timed as an interval of its own
  HIP_TRY(c, mark(c, CELLS_BEGIN));
  if (planeCorners)
    HIP_TRY(c, hipMemcpyAsync(w.points + 3 * nV, c->extPts, planeCorners * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(c, launch_emit_cells(w, c->g, c->prm.triangles, c->prm.q1, point_id_offset, nQ, needPlane ? c->extIds : nullptr,
                               nullptr, 0, 0, 0, s));
  if ((rc = launch_cell_attrs(c, point_id_offset, nV, nQ, false)) != CUBERILLE_OK) return rc;
  HIP_TRY(c, mark(c, END));
  if ((rc = component_count_to_host(c)) != CUBERILLE_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->hostTotals, w.totals, sizeof(Totals), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return finish_result(c, res);
}

}  // extern "C"

namespace {

// Everything of a step behind the sweep, launched without waiting: count + scan (+ gate), and the part of the emit that
// needs no id offset.  The slab's bit volume and slice occupancy are complete on the stream when this is called.
int step_launch(cuberille_ctx *c, const void **dev_row, size_t *row_bytes) {
  int rc;
  // blind launches need: the sizes of a previous extraction on this context, the default projection branch and every
  // scratch table (the vertex-word queue is set up by count_prepare; the others are checked below)
  const bool blind = c->haveHistory && c->w.vqueue && !c->tune.no_cmap && !c->tune.no_heads && c->tune.points_variant == 3 &&
                     (!c->prm.project || (c->prm.variant == CUBERILLE_PROJECT_DEFAULT && c->prm.gradVariant == 0 && !c->holdGradient &&
                                          c->countBsBits == 0)) &&
                     c->histV + c->histV / 4 < 0xfffff000ULL;
  if (blind) {
    Gate gate{};
    gate.on = 1;
    gate.coverV = c->histV + c->histV / 4 + 4096;
    gate.coverQ = c->histQ + c->histQ / 4 + 4096;
    const u64 vw = (u64)c->histVW + c->histVW / 4 + 1024;
    gate.coverVW = (u32)(vw < c->nwords ? vw : c->nwords);
    rc = count_launch(c, gate);
    if (rc) return rc;
    rc = emit_points_phase(c, true, true, gate.coverV, gate.coverQ, gate.coverVW);
    if (rc == CUBERILLE_OK) {
      c->stepMode = 1;
    } else {
      // a table could not be had: the count is in flight all the same, read it and go on by the exact sizes
      c->pointsEmitted = false;
      rc = totals_to_host(c);
      if (rc) return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      adopt_totals(c, nullptr, nullptr);
      // (Totals::go was set by the gate: a count that fits it may have let nothing run, the exact launches below do not ask)
    }
  } else {
    rc = count_finish(c, nullptr, nullptr);
    if (rc) return rc;
  }
  if (c->stepMode != 1) {
    // sized by a host read (the first extraction on a context, a fallback configuration): the vertex phase unless a
    // quirk-Q1 flag says that the counts may still change
    // (a source slice in this slab's own halo -- aliasMustResolve -- means a recount for certain; "nothing in my buffer
    //  below my first occupied slice" is an assumption the count has made already and the rows of the ranks below usually
    //  confirm: the vertex phase runs on it, the cell pass decides from the rows -- row_flags)
    c->stepMode = 2;
    if (!c->aliasMustResolve) {
      rc = emit_points_phase(c, true);
      if (rc) return rc;
    }
  }
  c->pointsStartedEarly = true;   // (the cells follow the host's gather of the rows, also where the vertex phase waits)
  *dev_row = c->w.totals;
  *row_bytes = sizeof(Totals);
  return CUBERILLE_OK;
}

// cuberille_step_begin, and the first half of cuberille_extract_device (the one-wait step with the context as its only rank:
// a whole volume, so an implied border is at home there while the steps of a driver's ranks refuse it)
int step_begin_impl(cuberille_ctx *c, const cuberille_image_desc *img, const void *dev_voxels, const cuberille_params *prm,
                    const cuberille_slab *slab, const View &view, const void **dev_row, size_t *row_bytes) {
  // (the caller has passed validate() and resolved the view)
  if (!dev_row || !row_bytes) return fail(c, CUBERILLE_ERR_ARGUMENT, "null row pointer");
  int rc = count_prepare(c, img, dev_voxels, prm, slab, view);
  if (rc) return rc;
  rc = classify_slab(c, img, slab);
  if (rc) return rc;
  return step_launch(c, dev_row, row_bytes);
}

}  // namespace

extern "C" {

// ---- one step without a host round trip between count and emit (the multi-GPU steady state) -------------------------
int cuberille_step_begin(cuberille_ctx *c, const cuberille_image_desc *img, const void *dev_voxels, const cuberille_params *prm,
                         const cuberille_slab *slab, const void **dev_row, size_t *row_bytes) {
  View view;
  int rc = validate(c, img, dev_voxels, prm, ROUTE_STEP);
  if (!rc) rc = view_of(c, img, prm, ROUTE_STEP, &view);
  return rc ? rc : step_begin_impl(c, img, dev_voxels, prm, slab, view, dev_row, row_bytes);
}

int cuberille_step_classify(cuberille_ctx *c, const cuberille_image_desc *img, const void *dev_voxels, const cuberille_params *prm,
                            const cuberille_slab *slab, uint64_t **dev_bits, size_t *words_per_slice) {
  View view;
  int rc = validate(c, img, dev_voxels, prm, ROUTE_STEP);
  if (!rc) rc = view_of(c, img, prm, ROUTE_STEP, &view);
  if (rc) return rc;
  if (!dev_bits || !words_per_slice) return fail(c, CUBERILLE_ERR_ARGUMENT, "null bit-plane pointer");
  rc = count_prepare(c, img, dev_voxels, prm, slab, view);
  if (rc) return rc;
  if (slab && slab->voxels_ready_event) HIP_TRY(c, hipStreamWaitEvent(c->stream, (hipEvent_t)slab->voxels_ready_event, 0));
  HIP_TRY(c, launch_classify(img->pixel_type, c->w, c->g, c->prm, c->g.oz0, c->g.oz1, c->tune, c->stream));
  c->stepMode = 3;
  *dev_bits = (uint64_t *)c->bits.p;
  *words_per_slice = (size_t)c->g.ny * c->g.W;
  return CUBERILLE_OK;
}

int cuberille_step_count(cuberille_ctx *c, void *halo_bits_event, void *halo_voxels_event, const void **dev_row, size_t *row_bytes) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (!dev_row || !row_bytes) return fail(c, CUBERILLE_ERR_ARGUMENT, "null row pointer");
  if (c->stepMode != 3) return fail(c, CUBERILLE_ERR_STATE, "cuberille_step_count follows cuberille_step_classify");
  HIP_TRY(c, hipSetDevice(c->device));
  c->stepMode = 0;
  if (halo_bits_event) HIP_TRY(c, hipStreamWaitEvent(c->stream, (hipEvent_t)halo_bits_event, 0));
  // which of the halo slices hold an inside voxel (quirk Q1 looks at it): from the planes that came in
  HIP_TRY(c, launch_occupancy_range(c->w, c->g, 0, c->g.oz0, c->stream));
  HIP_TRY(c, launch_occupancy_range(c->w, c->g, c->g.oz1, c->g.nzb, c->stream));
  c->voxelHaloEvent = (hipEvent_t)halo_voxels_event;
  const int rc = step_launch(c, dev_row, row_bytes);
  if (rc) c->voxelHaloEvent = nullptr;
  return rc;
}

}  // extern "C"

namespace {

// base: added to the offset summed from the rows (cuberille_extract_device on a slab: the caller's point_id_offset)
int step_end_impl(cuberille_ctx *c, const void *dev_rows, int n_ranks, int rank, u64 base, cuberille_result *res) {
  if (!c || !dev_rows || n_ranks < 1 || rank < 0 || rank >= n_ranks) return c ? fail(c, CUBERILLE_ERR_ARGUMENT, "bad rows or rank") : CUBERILLE_ERR_ARGUMENT;
  if (c->stepMode == 0) return fail(c, CUBERILLE_ERR_STATE, "cuberille_step_end follows cuberille_step_begin");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const bool blind = c->stepMode == 1;
  if (c->hostRowsCap < (size_t)n_ranks) {
    if (c->hostRows) (void)hipHostFree(c->hostRows);
    c->hostRows = nullptr;
    c->hostRowsCap = 0;
    HIP_TRY(c, hipHostMalloc((void **)&c->hostRows, (size_t)n_ranks * sizeof(Totals), hipHostMallocDefault));
    c->hostRowsCap = (size_t)n_ranks;
  }
  HIP_TRY(c, mark(c, CELLS_BEGIN));
  // the cells, unless a flag stands somewhere (the kernel looks at the rows itself: every rank decides alike).  Sized
  // by the cover values (blind) or by this rank's counts; a rank whose vertex phase did not run launches nothing.
  if (blind || c->pointsEmitted) {
    const u64 nQ = blind ? c->histQ + c->histQ / 4 + 4096 : c->tot.totQ - c->tot.Q0;
    HIP_TRY(c, launch_emit_cells(c->w, c->g, c->prm.triangles, c->prm.q1, base, nQ, nullptr, (const Totals *)dev_rows, n_ranks, rank,
                                 blind ? 1 : 0, s));
    // (the one-call routes alone come here with an attribute, the context their only rank; blind, its rows are sized by the gate's cover)
    const u64 nV = blind ? c->histV + c->histV / 4 + 4096 : c->tot.totV;
    if (const int rc = launch_cell_attrs(c, base, nV, nQ, blind)) return rc;
  }
  HIP_TRY(c, mark(c, END));
  if (const int rc = component_count_to_host(c)) return rc;   // (a flagged step leaves K unread)
  if (const int rc = totals_to_host(c)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->hostRows, dev_rows, (size_t)n_ranks * sizeof(Totals), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));                  // the one wait of the step
  u32 flags = 0;
  u64 off = base;
  for (int r = 0; r < n_ranks; r++) {
    flags |= row_flags(c->hostRows, r);                      // (the rule the cell pass applied on the device)
    if (r < rank) off += c->hostRows[r].totV - c->hostRows[r].V0;
  }
  const u32 mine = c->hostTotals->err;
  if (blind) {
    const bool ran = c->hostTotals->go != 0;
    adopt_totals(c, nullptr, nullptr);
    c->pointsEmitted = ran;                             // (a gate that said no: nothing ran, nothing is valid)
    if (!ran) c->pointsStartedEarly = false;
  } else {
    c->tot.nEscaped = c->hostTotals->nEscaped;
    c->tot.err = c->hostTotals->err;
  }
  c->escapeChecked = c->pointsEmitted;
  c->stepMode = 0;
  if (flags) {
    // nothing was written; the count stands and the synchronous calls take over from it (slab_info, recount,
    // emit_points, escaped_count / reproject_escaped, emit)
    (void)mine;
    c->err = "cuberille_step_end: a flag stands on some rank (quirk Q1 across slabs, capacity, or a walk left a thin halo)";
    if (res) *res = c->res;                             // the counts (what cuberille_count would have returned)
    return CUBERILLE_RETRY;
  }
  c->slabMesh = off != 0 || c->tot.V0 != 0 || part_of_a_volume(c->g);
  c->pointOffset = off;
  return finish_result(c, res);
}

}  // namespace

extern "C" {

int cuberille_step_end(cuberille_ctx *c, const void *dev_rows, int n_ranks, int rank, cuberille_result *res) {
  return step_end_impl(c, dev_rows, n_ranks, rank, 0, res);
}

int cuberille_failed_row(void *host_row, size_t capacity, size_t *row_bytes) {
  if (row_bytes) *row_bytes = sizeof(Totals);
  if (!host_row || capacity < sizeof(Totals)) return CUBERILLE_ERR_ARGUMENT;
  Totals t{};
  t.aliasZ = t.topZ = t.top2Z = -1;
  t.err = ERRF_RANK_FAILED;        // counts of zero: the ranks above add nothing to their offsets, and write nothing anyway
  std::memcpy(host_row, &t, sizeof t);
  return CUBERILLE_OK;
}

}  // extern "C"

namespace {

int extract_device_impl(cuberille_ctx *c, const cuberille_image_desc *img, const void *dev_voxels, const cuberille_params *prm,
                        const cuberille_slab *slab, const View &view, cuberille_result *res) {
  // the one-wait step with this context as the only rank: the first extraction on a context reads its counts back
  // before it sizes the emit, the following ones launch everything blindly from the sizes of the one before and wait
  // once (every volume the reference ships is in the regime where the waits ARE the extraction time)
  const void *row = nullptr;
  size_t rowBytes = 0;
  struct OneCall {
    cuberille_ctx *c;
    explicit OneCall(cuberille_ctx *ctx) : c(ctx) { c->oneCall = true; }
    ~OneCall() { c->oneCall = false; }
  } guard(c);
  int rc = step_begin_impl(c, img, dev_voxels, prm, slab, view, &row, &rowBytes);
  if (rc) return rc;
  rc = step_end_impl(c, row, 1, 0, slab ? slab->point_id_offset : 0, res);
  if (rc != CUBERILLE_RETRY) return rc;
  // counts beyond the guess, or a slab that needs its neighbours (quirk Q1, an escaped walk): the count stands
  return cuberille_emit(c, slab ? slab->point_id_offset : 0, res);
}

}  // namespace

extern "C" {

int cuberille_extract_device(cuberille_ctx *c, const cuberille_image_desc *img, const void *dev_voxels,
                             const cuberille_params *prm, const cuberille_slab *slab, cuberille_result *res) {
  View view;
  int rc = validate(c, img, dev_voxels, prm);
  if (!rc) rc = view_of(c, img, prm, whole_volume(slab) ? ROUTE_DEVICE : ROUTE_SLAB, &view);
  return rc ? rc : extract_device_impl(c, img, dev_voxels, prm, slab, view, res);
}

}  // extern "C"

namespace {

// The pinned staging ring of the chunked copies (two slots of `bytes`, their events, the copy stream), (re)made in one
// place: the recorded size only ever describes two live slots.
int ensure_staging(cuberille_ctx *c, size_t bytes) {
  if (!c->copyStream) HIP_TRY(c, hipStreamCreateWithFlags(&c->copyStream, hipStreamNonBlocking));
  for (int i = 0; i < 2; i++) {
    if (!c->stageFree[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->stageFree[i], hipEventDisableTiming));
    if (!c->chunkIn[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->chunkIn[i], hipEventDisableTiming));
  }
  if (c->stageBytes >= bytes && c->stage[0] && c->stage[1]) return CUBERILLE_OK;
  c->stageBytes = 0;
  for (int i = 0; i < 2; i++)
    if (c->stage[i]) { (void)hipHostFree(c->stage[i]); c->stage[i] = nullptr; }
  for (int i = 0; i < 2; i++) {
    if (g_fail_alloc_countdown >= 0 && g_fail_alloc_countdown-- == 0)
      return fail(c, CUBERILLE_ERR_HIP, "hipHostMalloc(staging slot): out of memory (failure drill)");
    HIP_TRY(c, hipHostMalloc(&c->stage[i], bytes, hipHostMallocDefault));
  }
  c->stageBytes = bytes;
  return CUBERILLE_OK;
}

// Let what is in flight finish before the staging slots are written again (a chunked copy that failed half way).
void drain(cuberille_ctx *c) {
  (void)hipStreamSynchronize(c->copyStream);
  (void)hipStreamSynchronize(c->stream);
}

// Host threads that move the chunks of `total` bytes between pageable memory and the pinned staging slots, each one a fixed
// share of every chunk (a single memcpy stream cannot feed a PCIe Gen5 link; a handful can).  move(i, a, b) moves bytes
// [a, b) of chunk i; the threads take chunk i once release(i) has been called, and wait(i) returns when all of them are
// done with it.  Destruction lets them finish what has been released and joins them.
// threads: 0 = the rule of one context (8 where the host has 16 cores or more).
int pool_threads_default() {
  const unsigned hw = std::thread::hardware_concurrency();
  return (int)(hw >= 16 ? 8 : (hw >= 4 ? hw / 2 : 1));
}

struct StagePool {
  template <class Move>
  StagePool(size_t total, size_t chunk, Move move, int threads = 0) : done_((total + chunk - 1) / chunk) {
    n_ = threads > 0 ? threads : pool_threads_default();
    for (auto &d : done_) d.store(0);
    for (int t = 0; t < n_; t++)
      threads_.emplace_back([this, t, total, chunk, move] {
        for (size_t i = 0; i < done_.size(); i++) {
          while (released_.load(std::memory_order_acquire) < (long long)i) {
            // (the destructor follows the last release at once: a thread that read released_ just before that release and
            //  abort_ just after the destructor's store must look again, or it leaves without moving its share of the last
            //  chunk -- the destination then keeps whatever the memory held)
            if (abort_.load(std::memory_order_acquire)) {
              if (released_.load(std::memory_order_acquire) >= (long long)i) break;
              return;
            }
            std::this_thread::yield();
          }
          const size_t cb = total - i * chunk < chunk ? total - i * chunk : chunk;
          const size_t a = cb * t / n_ & ~(size_t)63, b = (t == n_ - 1) ? cb : (cb * (t + 1) / n_ & ~(size_t)63);
          move(i, a, b);
          done_[i].fetch_add(1, std::memory_order_release);
        }
      });
  }
  ~StagePool() {
    abort_.store(true);
    for (auto &t : threads_) t.join();
  }
  void release(size_t i) { released_.store((long long)i, std::memory_order_release); }
  void wait(size_t i) { while (done_[i].load(std::memory_order_acquire) < n_) std::this_thread::yield(); }
  int n_ = 1;
  std::atomic<long long> released_{-1};     // the threads may take every chunk i <= released_
  std::atomic<bool> abort_{false};
  std::vector<std::atomic<int>> done_;      // per chunk: threads that have moved their share
  std::vector<std::thread> threads_;
};

// The count of a volume uploaded in chunks through the staging slots (of stageBytes): chunk i (slices [z0, z1)) goes
// through slot i & 1 -- wait until the slot is free (chunk i - 2 has crossed the link), fill it (fill(i, slot, z0, z1): 0,
// or the status with which the caller's source gave up), copy it on the copy stream, threshold it on the context's stream
// once it has landed.  img describes the buffer (slab: its place in the volume, or null for a whole one); every slice of
// the buffer is thresholded, as classify_slab does.  The caller emits.
template <class Fill>
int extract_chunked(cuberille_ctx *c, const cuberille_image_desc *img, const cuberille_params *prm, const cuberille_slab *slab,
                    const View &view, size_t stageBytes, size_t slicesPerChunk, const char *what, Fill fill) {
  int rc = ensure_staging(c, stageBytes);
  if (rc) return rc;
  rc = count_prepare(c, img, c->voxOwn.p, prm, slab, view);
  if (rc) return rc;
  const size_t sliceBytes = (size_t)img->dims[0] * img->dims[1] * pixel_size(img->pixel_type), nz = (size_t)img->dims[2];
  hipError_t e = hipSuccess;
  int gaveUp = 0;
  for (size_t i = 0; i * slicesPerChunk < nz; i++) {
    const size_t z0 = i * slicesPerChunk, z1 = z0 + slicesPerChunk < nz ? z0 + slicesPerChunk : nz;
    void *slot = c->stage[i & 1];
    if (i >= 2 && (e = hipEventSynchronize(c->chunkIn[i & 1])) != hipSuccess) break;
    if ((gaveUp = fill(i, slot, z0, z1)) != 0) break;
    e = hipMemcpyAsync((char *)c->voxOwn.p + z0 * sliceBytes, slot, (z1 - z0) * sliceBytes, hipMemcpyHostToDevice, c->copyStream);
    if (e == hipSuccess) e = hipEventRecord(c->chunkIn[i & 1], c->copyStream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->chunkIn[i & 1], 0);
    if (e == hipSuccess) e = launch_classify(c->pixel_type, c->w, c->g, c->prm, (int)z0, (int)z1, c->tune, c->stream);
    if (e != hipSuccess) break;
  }
  if (e != hipSuccess || gaveUp) {
    drain(c);
    if (gaveUp) return fail(c, CUBERILLE_ERR_SOURCE, "the chunk source gave up with status " + std::to_string(gaveUp));
    return fail(c, CUBERILLE_ERR_HIP, std::string(what) + hipGetErrorString(e));
  }
  return count_finish(c, nullptr, nullptr);
}

// Large volumes from pageable host memory: z-chunks of whole slices; chunk i is thresholded on the context's stream while
// chunk i+1 crosses the link and the host threads (c->poolThreads) stage chunk i+2.  The buffer (img) starts `base` bytes
// into host_voxels.
// srcRowBytes / srcSliceBytes (cuberille_set_region): the buffer (img) is a box of the caller's image whose rows and slices
// lie that far apart in host memory, `base` its first voxel -- the staging threads gather the box's rows of each chunk straight
// from the caller's image, no host-side crop exists; 0: the buffer is contiguous there.
// chunkBytes: 0 = kUploadChunk (Tuning::upload_chunk_kib: smaller chunks, for tests of the pipeline on small volumes).
constexpr size_t kUploadChunk = 32u << 20;
int count_host_chunked(cuberille_ctx *c, const cuberille_image_desc *img, const void *host_voxels, size_t base,
                       const cuberille_params *prm, const cuberille_slab *slab, const View &view, size_t srcRowBytes = 0,
                       size_t srcSliceBytes = 0, size_t chunkBytes = 0) {
  const size_t rowBytes = (size_t)img->dims[0] * pixel_size(img->pixel_type), ny = (size_t)img->dims[1];
  const size_t sliceBytes = rowBytes * ny;
  const size_t bytes = sliceBytes * (size_t)img->dims[2];
  size_t want = kUploadChunk;
  if (chunkBytes && chunkBytes < kUploadChunk) want = chunkBytes < sliceBytes ? sliceBytes : chunkBytes;   // (the test switch: a slice at least)
  const size_t slices = want / sliceBytes;
  if (slices < 1) return fail(c, CUBERILLE_ERR_LIMIT, "a slice of the image does not fit a chunk of the upload pipeline");   // (the callers' rule)
  const size_t chunk = slices * sliceBytes;
  const char *src = (const char *)host_voxels + base;
  StagePool pool(bytes, chunk, [&](size_t i, size_t a, size_t b) {
    char *dst = (char *)c->stage[i & 1];
    if (!srcRowBytes) {
      std::memcpy(dst + a, src + i * chunk + a, b - a);
      return;
    }
    for (size_t off = i * chunk + a, end = i * chunk + b; off < end;) {     // bytes [off, end) of the box, row piece by row piece
      const size_t r = off / rowBytes, o = off - r * rowBytes, n = rowBytes - o < end - off ? rowBytes - o : end - off;
      const size_t z = r / ny, y = r - z * ny;
      std::memcpy(dst + (off - i * chunk), src + z * srcSliceBytes + y * srcRowBytes + o, n);
      off += n;
    }
  }, c->poolThreads);
  return extract_chunked(c, img, prm, slab, view, kUploadChunk, slices, "overlapped upload: ",
                         [&](size_t i, void *, size_t, size_t) {
                           pool.release(i);
                           pool.wait(i);
                           return 0;
                         });
}

// Where the size rule of cuberille_extract_host sends a buffer of these dimensions: the chunk pipeline (a GiB and more, slices
// that fit a chunk) or one plain copy.
bool upload_in_chunks(size_t sliceBytes, size_t bytes) { return bytes >= (1ull << 30) && sliceBytes <= kUploadChunk; }

int extract_host_impl(cuberille_ctx *c, const cuberille_image_desc *img, const void *host_voxels, const cuberille_params *prm,
                      View view, cuberille_result *res) {
  HIP_TRY(c, hipSetDevice(c->device));
  // VIEW_REGION: only the box crosses the link, straight from the caller's image -- the device copy is the box, contiguous,
  // and from here on the image IS the box (its description cuberille_region_desc's) under the view that says so
  const bool box = view.kind == VIEW_REGION;
  const cuberille_image_desc whole = *img, cut = framed_desc(view, img);
  const size_t at[3] = {(size_t)view.start[0], (size_t)view.start[1], (size_t)view.start[2]};
  if (box) { img = &cut; view = applied_region(cut); }
  const size_t pix = pixel_size(img->pixel_type);
  const size_t sliceBytes = (size_t)img->dims[0] * img->dims[1] * pix;
  const size_t bytes = sliceBytes * (size_t)img->dims[2];
  const size_t srcRow = (size_t)whole.dims[0] * pix, srcSlice = srcRow * (size_t)whole.dims[1];
  const size_t base = box ? at[0] * pix + at[1] * srcRow + at[2] * srcSlice : 0;
  const bool rowsApart = box && (img->dims[0] != whole.dims[0] || img->dims[1] != whole.dims[1]);
  HIP_TRY(c, c->voxOwn.reserve(bytes));
  // below a GiB: one plain copy (the runtime stages pageable memory itself, at link rate once the copy is large; the
  // chunk pipeline below needs some tens of chunks to amortise its start -- measured 34 ms against 11 ms at 512^3 f32);
  // the extraction follows on the stream
  const bool chunks = c->tune.upload_chunk_kib > 0 ? sliceBytes <= kUploadChunk : upload_in_chunks(sliceBytes, bytes);
  if (!chunks) {
    if (rowsApart) {
      // (one strided copy: the box's rows from the caller's image into the contiguous device buffer)
      hipMemcpy3DParms cp{};
      cp.srcPtr = make_hipPitchedPtr(const_cast<char *>((const char *)host_voxels + base), srcRow, srcRow, (size_t)whole.dims[1]);
      cp.dstPtr = make_hipPitchedPtr(c->voxOwn.p, (size_t)img->dims[0] * pix, (size_t)img->dims[0] * pix, (size_t)img->dims[1]);
      cp.extent = make_hipExtent((size_t)img->dims[0] * pix, (size_t)img->dims[1], (size_t)img->dims[2]);
      cp.kind = hipMemcpyHostToDevice;
      HIP_TRY(c, hipMemcpy3DAsync(&cp, c->stream));
    } else {
      HIP_TRY(c, hipMemcpyAsync(c->voxOwn.p, (const char *)host_voxels + base, bytes, hipMemcpyHostToDevice, c->stream));
    }
    return extract_device_impl(c, img, c->voxOwn.p, prm, nullptr, view, res);
  }
  const int rc = count_host_chunked(c, img, host_voxels, base, prm, nullptr, view, rowsApart ? srcRow : 0, rowsApart ? srcSlice : 0,
                          (size_t)(c->tune.upload_chunk_kib > 0 ? c->tune.upload_chunk_kib : 0) << 10);
  return rc ? rc : cuberille_emit(c, 0, res);
}

}  // namespace

extern "C" {

int cuberille_extract_host(cuberille_ctx *c, const cuberille_image_desc *img, const void *host_voxels,
                           const cuberille_params *prm, cuberille_result *res) {
  View view;
  int rc = validate(c, img, host_voxels, prm);
  if (!rc) rc = view_of(c, img, prm, ROUTE_HOST, &view);
  return rc ? rc : extract_host_impl(c, img, host_voxels, prm, view, res);
}

int cuberille_extract_stream(cuberille_ctx *c, const cuberille_image_desc *img, cuberille_chunk_source source, void *user,
                             const cuberille_params *prm, cuberille_result *res) {
  if (c && !source) return fail(c, CUBERILLE_ERR_ARGUMENT, "null chunk source");
  View view;
  int rc = validate(c, img, (const void *)source, prm);
  if (!rc) rc = view_of(c, img, prm, ROUTE_STREAM, &view);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t sliceBytes = (size_t)img->dims[0] * img->dims[1] * pixel_size(img->pixel_type);
  HIP_TRY(c, c->voxOwn.reserve(sliceBytes * (size_t)img->dims[2]));
  // chunks of about 32 MiB, whole slices, at least one; the caller's source fills each slot on this thread, in order
  const size_t slicesPerChunk = sliceBytes >= (32u << 20) ? 1 : (32u << 20) / sliceBytes;
  rc = extract_chunked(c, img, prm, nullptr, view, slicesPerChunk * sliceBytes, slicesPerChunk, "streamed upload: ",
                       [&](size_t, void *slot, size_t z0, size_t z1) { return source(user, slot, (int64_t)z0, (int64_t)z1); });
  return rc ? rc : cuberille_emit(c, 0, res);
}

int cuberille_warm_up(cuberille_ctx *c, const cuberille_image_desc *img, const cuberille_params *prm) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  cuberille_params dflt{};
  dflt.iso_value = 1.0; dflt.generate_triangles = 1; dflt.project_vertices = 1; dflt.distance_threshold = 0.5;
  dflt.step_length = -1.0; dflt.relaxation = 0.95; dflt.max_steps = 50; dflt.emulate_empty_slice_aliasing = 1;
  dflt.iso_value_int = 1;
  // A count, a mesh or an open step on the context: its workspace is in use -- the toy extraction would replace the state,
  // and DevBuf::reserve frees before it allocates, which would leave the workspace pointers of the live count (c->w, the
  // bit volume) dangling under cuberille_emit / _recount / _slice_bits_device / _alias_plane_device / _debug_bits.
  // Such a context has run kernels already; the next extraction grows what it needs itself.
  const bool live = c->counted || c->haveMesh || c->stepMode != 0;
  if (live) c->warm = true;
  if (!c->warm) {
    // one tiny extraction: the first launch of any kernel loads the library's code objects, the first copies and events
    // set up the runtime's queues.  8 x 8 x 8 voxels with a 4 x 4 x 4 block inside; nothing of it stays on the context.
    unsigned char tiny[512];
    for (int z = 0; z < 8; z++)
      for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++) tiny[(z * 8 + y) * 8 + x] = (x >= 2 && x < 6 && y >= 2 && y < 6 && z >= 2 && z < 6) ? 200 : 0;
    cuberille_image_desc d{};
    d.pixel_type = CUBERILLE_PIX_U8;
    for (int i = 0; i < 3; i++) { d.dims[i] = 8; d.spacing[i] = 1.0; d.direction[i * 4] = 1.0; }
    cuberille_params p = dflt;
    p.iso_value = 100.0;
    cuberille_result r{};
    for (int i = 0; i < 2; i++) {            // twice: the second one takes the blind launches of the one-wait step
      // (the whole toy volume: the context's view settings speak of the caller's volumes, not of this one)
      const int rc = extract_host_impl(c, &d, tiny, &p, View{}, &r);
      if (rc) return rc;
    }
    // the runtime sets up its staging for copies from and to PAGEABLE memory at the first copy that needs it (measured
    // through the reference's driver: 7.2 ms inside the first hipMemcpyAsync of nucleon.mha's 69 KB, profiles/
    // r4_cold_update.log): one round trip of a size that takes its staging buffers, one of a size it pins in place
    {
      std::vector<char> host(8u << 20, 1);
      HIP_TRY(c, c->voxOwn.reserve(host.size()));
      const size_t sizes[2] = {256u << 10, host.size()};
      for (size_t n : sizes) {
        HIP_TRY(c, hipMemcpyAsync(c->voxOwn.p, host.data(), n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(host.data(), c->voxOwn.p, n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
      }
    }
    c->haveHistory = false;                  // (sizes of a toy volume: the first real extraction reads its own counts)
    c->haveMesh = false;
    for (auto &a : c->attr) a.have = false;
    c->ps.have = false;
    c->counted = false;
    c->warm = true;
  }
  if (!img) return CUBERILLE_OK;
  if (pixel_size(img->pixel_type) == 0) return fail(c, CUBERILLE_ERR_ARGUMENT, "unknown pixel type");
  for (int i = 0; i < 3; i++)
    if (img->dims[i] < 1 || img->dims[i] > 0x7fffffffLL) return fail(c, CUBERILLE_ERR_ARGUMENT, "image dimensions out of range");
  (void)prm;
  if (live) return CUBERILLE_OK;
  // the buffers whose size follows from the description (count_prepare, emit_points_phase, cuberille_extract_host); a
  // reservation that fails here is asked for again, and reported, by the extraction
  // (VIEW_BORDER: the workspace of the image with its ring, the voxel buffer of the image as it is)
  // (VIEW_REGION: the workspace AND the voxel buffer of the box -- cuberille_extract_host uploads nothing else)
  View view;
  const int vrc = view_of(c, img, &dflt, ROUTE_WARM_UP, &view);
  if (vrc) return vrc;
  const cuberille_image_desc framed = framed_desc(view, img);
  const Grid g = whole_grid(&framed, c->tune);
  const CountSizes sz = count_sizes(g, c->tune, view);
  const cuberille_image_desc *held = view.kind == VIEW_REGION ? &framed : img;     // the image a host-resident extraction keeps on the device
  const size_t bytes = (size_t)held->dims[0] * (size_t)held->dims[1] * (size_t)held->dims[2] * pixel_size(img->pixel_type);
  const std::pair<DevBuf *, size_t> want[] = {{&c->voxOwn, bytes}, {&c->bits, sz.bits}, {&c->occ, sz.occ}, {&c->prefix, sz.prefix},
                                              {&c->segPre, sz.segPre}, {&c->blockTot, sz.blockTot}, {&c->blockBase, sz.blockBase},
                                              {&c->flatBits, sz.flatBits}, {&c->vqueue, sz.vqueue}, {&c->cmap, cmap_bytes(g, c->tune)}};
  bool ok = true;
  for (const auto &b : want)   // (0 bytes: not wanted, nothing to reserve)
    if (b.first->reserve(b.second) != hipSuccess) { ok = false; break; }
  if (!ok) (void)hipGetLastError();
  // the pinned staging ring: a chunked upload (volumes of a GiB and more) and the download of a mesh of more than 128 MiB
  // go through it; a volume of 64 MiB can carry such a mesh
  if (ok && bytes >= (64ull << 20)) (void)ensure_staging(c, 32u << 20);
  return CUBERILLE_OK;
}

int cuberille_slice_counts(cuberille_ctx *c, uint64_t *points, uint64_t *quads, size_t n_slices) {
  if (!c || (!points && !quads)) return CUBERILLE_ERR_ARGUMENT;
  if (!c->counted && !c->haveMesh) return fail(c, CUBERILLE_ERR_STATE, "no count on this context");
  const int own = c->g.oz1 - c->g.oz0, counted = c->g.oz1 - c->g.cz0;
  if (n_slices != (size_t)own) return fail(c, CUBERILLE_ERR_ARGUMENT, "one entry per owned slice, please");
  HIP_TRY(c, hipSetDevice(c->device));
  // (scratch: the cell buffer is free between a count and its emit, but a mesh may be in it; a small buffer of its own)
  DevBuf tmp;
  HIP_TRY(c, tmp.reserve((size_t)(counted + 1) * 2 * sizeof(u64)));
  std::vector<u64> host((size_t)(counted + 1) * 2);
  hipError_t e = launch_slice_prefix(c->w, c->g, (u64 *)tmp.p, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(host.data(), tmp.p, host.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  tmp.release();
  if (e != hipSuccess) return fail(c, CUBERILLE_ERR_HIP, std::string("slice counts: ") + hipGetErrorString(e));
  const int skip = c->g.oz0 - c->g.cz0;                       // the ghost slice
  for (int z = 0; z < own; z++) {
    if (points) points[z] = host[2 * (size_t)(z + skip + 1)] - host[2 * (size_t)(z + skip)];
    if (quads) quads[z] = host[2 * (size_t)(z + skip + 1) + 1] - host[2 * (size_t)(z + skip) + 1];
  }
  return CUBERILLE_OK;
}

int cuberille_slab_info(cuberille_ctx *c, cuberille_slab_status *out) {
  if (!c || !out) return CUBERILLE_ERR_ARGUMENT;
  if ((!c->counted && !c->haveMesh) || !c->slabMode || !c->hostOcc)
    return fail(c, CUBERILLE_ERR_STATE, "no counted slab on this context");
  out->alias_source_below_buffer = c->aliasBelowBuffer ? 1 : 0;
  out->reserved = 0;
  out->lowest_occupied_z = out->highest_occupied_z = out->second_highest_occupied_z = -1;
  for (int z = c->g.oz0; z < c->g.oz1; z++)
    if (c->hostOcc[(size_t)z]) {
      if (out->lowest_occupied_z < 0) out->lowest_occupied_z = c->g.zglob0 + z;
      out->second_highest_occupied_z = out->highest_occupied_z;
      out->highest_occupied_z = c->g.zglob0 + z;
    }
  out->alias_z = c->aliasZ >= 0 ? c->g.zglob0 + c->aliasZ : -1;
  return CUBERILLE_OK;
}

static bool set_opt(Tuning &t, const char *name, long long v) {
#define OPT(field) if (!std::strcmp(name, #field)) { t.field = (int)v; return true; }
  OPT(no_cmap) OPT(no_heads) OPT(no_vqueue) OPT(no_stream_classify) OPT(classify_variant) OPT(classify_grid)
  OPT(points_variant) OPT(points_no_split) OPT(count_variant) OPT(cmap_linear) OPT(proj_chunk) OPT(proj_waves) OPT(proj_refill) OPT(proj_xcd) OPT(proj_literal) OPT(stage_timing) OPT(classify_keep_tail) OPT(proj_chunk64_below) OPT(points_split) OPT(count_no_fold) OPT(proj_short) OPT(proj_ident) OPT(upload_chunk_kib)
#undef OPT
  return false;
}

int cuberille_debug_h2d_seconds(cuberille_ctx *c, size_t bytes, double *seconds) {
  if (!c || !seconds || !bytes) return CUBERILLE_ERR_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t piece = 64u << 20;
  void *host = nullptr, *dev = nullptr;
  HIP_TRY(c, hipHostMalloc(&host, piece, hipHostMallocDefault));
  if (hipMalloc(&dev, piece) != hipSuccess) { (void)hipHostFree(host); return fail(c, CUBERILLE_ERR_HIP, "hipMalloc failed"); }
  std::memset(host, 1, piece);
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t e = hipEventCreate(&a);
  if (e == hipSuccess) e = hipEventCreate(&b);
  if (e == hipSuccess) e = hipMemcpyAsync(dev, host, piece, hipMemcpyHostToDevice, c->stream);   // warm-up
  if (e == hipSuccess) e = hipEventRecord(a, c->stream);
  for (size_t done = 0; done < bytes && e == hipSuccess; done += piece)
    e = hipMemcpyAsync(dev, host, bytes - done < piece ? bytes - done : piece, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipEventRecord(b, c->stream);
  if (e == hipSuccess) e = hipEventSynchronize(b);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
  if (a) (void)hipEventDestroy(a);
  if (b) (void)hipEventDestroy(b);
  (void)hipFree(dev);
  (void)hipHostFree(host);
  if (e != hipSuccess) return fail(c, CUBERILLE_ERR_HIP, std::string("link measurement: ") + hipGetErrorString(e));
  *seconds = 1e-3 * ms;
  return CUBERILLE_OK;
}

int cuberille_debug_set_option(cuberille_ctx *c, const char *name, int64_t value) {
  if (!c || !name) return CUBERILLE_ERR_ARGUMENT;
  if (!std::strcmp(name, "defaults")) { c->tune = Tuning(); g_fail_alloc_countdown = -1; return CUBERILLE_OK; }
  if (!std::strcmp(name, "fail_alloc_at")) { g_fail_alloc_countdown = (long long)value; return CUBERILLE_OK; }
  if (!set_opt(c->tune, name, (long long)value)) return fail(c, CUBERILLE_ERR_ARGUMENT, std::string("unknown option ") + name);
  return CUBERILLE_OK;
}

int cuberille_mesh_device(const cuberille_ctx *c, const float **d_points, const uint64_t **d_cells) {
  if (!c || !c->haveMesh) return CUBERILLE_ERR_STATE;
  if (d_points) *d_points = (const float *)c->rows[ROW_POINTS].row.p + 3 * c->tot.V0;
  if (d_cells) *d_cells = (const uint64_t *)c->rows[ROW_CELLS].row.p;
  return CUBERILLE_OK;
}

}  // extern "C"

namespace {

// Device -> pageable host memory: 32 MiB chunks land in the pinned staging slots on the copy stream while a few host
// threads move the previous chunk to its destination.  What this buys is the FIRST touch of a freshly allocated
// destination (the usual case: one result array per extraction), which the page faults bound: 668 MB in 48 ms against
// 65 ms for one plain hipMemcpy on the same box; into memory that has been touched before both run at the link's
// 52-55 GB/s (12.9 against 12.2 ms).  Small copies take the plain way.
int download_pipelined(cuberille_ctx *c, void *dst, const void *src, size_t bytes) {
  const size_t kChunk = 32u << 20;
  if (bytes < 4 * kChunk) {
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CUBERILLE_OK;
  }
  if (const int rc = ensure_staging(c, kChunk)) return rc;
  // the mesh was written on the context's stream
  HIP_TRY(c, hipEventRecord(c->stageFree[0], c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->copyStream, c->stageFree[0], 0));
  const size_t nchunks = (bytes + kChunk - 1) / kChunk;
  auto chunkBytes = [&](size_t i) { return bytes - i * kChunk < kChunk ? bytes - i * kChunk : kChunk; };
  StagePool pool(bytes, kChunk, [&](size_t i, size_t a, size_t b) {
    std::memcpy((char *)dst + i * kChunk + a, (const char *)c->stage[i & 1] + a, b - a);
  }, c->poolThreads);
  auto issue = [&](size_t i) -> hipError_t {
    hipError_t e = hipMemcpyAsync(c->stage[i & 1], (const char *)src + i * kChunk, chunkBytes(i), hipMemcpyDeviceToHost, c->copyStream);
    if (e == hipSuccess) e = hipEventRecord(c->chunkIn[i & 1], c->copyStream);
    return e;
  };
  hipError_t e = issue(0);
  for (size_t i = 0; i < nchunks && e == hipSuccess; i++) {
    if (i + 1 < nchunks) {
      // slot (i + 1) & 1 held chunk i - 1: the host threads must be done with it
      if (i >= 1) pool.wait(i - 1);
      e = issue(i + 1);
      if (e != hipSuccess) break;
    }
    e = hipEventSynchronize(c->chunkIn[i & 1]);
    if (e == hipSuccess) pool.release(i);
  }
  if (e == hipSuccess) return CUBERILLE_OK;
  drain(c);
  return fail(c, CUBERILLE_ERR_HIP, std::string("mesh download: ") + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int cuberille_mesh_download(cuberille_ctx *c, float *points, uint64_t *cells) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (!c->haveMesh) return fail(c, CUBERILLE_ERR_STATE, "no mesh: call cuberille_extract_* or cuberille_emit first");
  HIP_TRY(c, hipSetDevice(c->device));
  const cuberille_result &r = c->res;
  if (points && r.n_points) {
    const int rc = download_pipelined(c, points, (const float *)c->row(ROW_POINTS).p + 3 * c->tot.V0, mesh_row_bytes(c, ROW_POINTS));
    if (rc) return rc;
  }
  if (cells && r.n_cells) {
    const int rc = download_pipelined(c, cells, c->row(ROW_CELLS).p, mesh_row_bytes(c, ROW_CELLS));
    if (rc) return rc;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CUBERILLE_OK;
}

int cuberille_mesh_host(cuberille_ctx *c, float **points, uint64_t **cells) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (!c->haveMesh) return fail(c, CUBERILLE_ERR_STATE, "no mesh: call cuberille_extract_* or cuberille_emit first");
  if (!c->hostMeshValid) {
    const size_t pb = mesh_row_bytes(c, ROW_POINTS), cb = mesh_row_bytes(c, ROW_CELLS);
    if (!c->hostPoints.reserve(pb ? pb : 1) || !c->hostCells.reserve(cb ? cb : 1))
      return fail(c, CUBERILLE_ERR_HIP, "cuberille_mesh_host: out of host memory");
    const int rc = cuberille_mesh_download(c, (float *)c->hostPoints.p, (uint64_t *)c->hostCells.p);
    if (rc) return rc;
    c->hostMeshValid = true;
  }
  if (points) *points = (float *)c->hostPoints.p;
  if (cells) *cells = (uint64_t *)c->hostCells.p;
  return CUBERILLE_OK;
}

// What the three setters share.  Off: the context holds what one that never heard of the setting holds -- the last mesh stays, the
// attribute's rows go with their partners (behind a keep, whichever of the two the extraction was sized for) and its scratch.
static int set_attr(cuberille_ctx *c, int a, int on, bool *released = nullptr) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (c->stepMode != 0) return fail(c, CUBERILLE_ERR_STATE, "a step is open on this context");
  c->attr[a].on = on != 0;
  if (on) return CUBERILLE_OK;
  std::vector<DevBuf *> held;
  if (a == ATTR_COMPONENTS) held.assign(c->compScratch, c->compScratch + 4);
  for (int r = 0; r < N_ROWS; r++)
    if (kRows[r].attr == a) { held.push_back(&c->rows[r].row); held.push_back(&c->rows[r].spare); }
  if (std::none_of(held.begin(), held.end(), [](const DevBuf *b) { return b->p != nullptr; })) return CUBERILLE_OK;
  (void)hipSetDevice(c->device);
  HIP_TRY(c, hipStreamSynchronize(c->stream));     // (the pass may still be writing them)
  for (DevBuf *b : held) b->release();
  c->attr[a].have = c->attr[a].counting = false;
  if (released) *released = true;
  return CUBERILLE_OK;
}

static int attr_preconditions(cuberille_ctx *c, int a) {
  if (!c->haveMesh) return fail(c, CUBERILLE_ERR_STATE, "no mesh: call cuberille_extract_* or cuberille_emit first");
  if (!c->attr[a].have) return fail(c, CUBERILLE_ERR_STATE, attr_missing(a));
  return CUBERILLE_OK;
}

int cuberille_set_point_normals(cuberille_ctx *c, int on) { return set_attr(c, ATTR_NORMALS, on); }

int cuberille_normals_device(cuberille_ctx *c, const float **d_normals) {
  if (!c || !d_normals) return CUBERILLE_ERR_ARGUMENT;
  *d_normals = nullptr;
  if (const int rc = attr_preconditions(c, ATTR_NORMALS)) return rc;
  *d_normals = (const float *)c->row(ROW_NORMALS).p;   // (a whole volume: no ghost vertices ahead of the owned ones; null with no point)
  return CUBERILLE_OK;
}

int cuberille_normals_download(cuberille_ctx *c, float *normals) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (const int rc = attr_preconditions(c, ATTR_NORMALS)) return rc;
  if (!c->res.n_points) return CUBERILLE_OK;
  if (!normals) return fail(c, CUBERILLE_ERR_ARGUMENT, "null output pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  return download_pipelined(c, normals, c->row(ROW_NORMALS).p, mesh_row_bytes(c, ROW_NORMALS));
}

// The point scalars' setter: what it releases when the setting goes off or the image is replaced -- the row with its spare, and
// the copy -- behind whatever may still be reading or writing them.
static int point_scalars_release(cuberille_ctx *c, bool rows) {
  PointScalars &ps = c->ps;
  if ((rows && (ps.rows.row.p || ps.rows.spare.p)) || ps.copy.p) {
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (rows) { ps.rows.row.release(); ps.rows.spare.release(); }
  ps.copy.release();
  ps.vox = nullptr;
  return CUBERILLE_OK;
}

int cuberille_set_point_scalars(cuberille_ctx *c, const cuberille_image_desc *img, const void *voxels, int location, double outside_value) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (c->stepMode != 0) return fail(c, CUBERILLE_ERR_STATE, "a step is open on this context");
  PointScalars &ps = c->ps;
  if (!img) {                                          // off: the context holds what one that never heard of the setting holds
    if (const int rc = point_scalars_release(c, true)) return rc;
    ps.on = ps.counting = ps.have = false;
    return CUBERILLE_OK;
  }
  // the description, by the rules of an input image (validate), in this setting's words; the setting stays as it was
  const std::string name = std::string(kPointScalarsNoun) + " (" + kPointScalarsFn + "): the second image's ";
  if (!voxels) return fail(c, CUBERILLE_ERR_ARGUMENT, name + "voxel pointer is null");
  if (location != CUBERILLE_MEM_HOST && location != CUBERILLE_MEM_DEVICE)
    return fail(c, CUBERILLE_ERR_ARGUMENT, name + "location is neither CUBERILLE_MEM_HOST nor CUBERILLE_MEM_DEVICE");
  if (pixel_size(img->pixel_type) == 0) return fail(c, CUBERILLE_ERR_ARGUMENT, name + "pixel type is unknown");
  for (int i = 0; i < 3; i++) {
    if (img->dims[i] < 1) return fail(c, CUBERILLE_ERR_ARGUMENT, name + "dimensions must be >= 1");
    if (img->dims[i] > 0x7fffffffLL) return fail(c, CUBERILLE_ERR_ARGUMENT, name + "dimension exceeds 2^31-1");
    if (!(img->spacing[i] > 0.0)) return fail(c, CUBERILLE_ERR_ARGUMENT, name + "spacing must be > 0");
    if (img->index_start[i] < -(1LL << 30) || img->index_start[i] > (1LL << 30))
      return fail(c, CUBERILLE_ERR_ARGUMENT, name + "start index must lie within +-2^30");
  }
  Geo geo{};
  Params unused{};
  const cuberille_params noParams{};
  resolve(img, &noParams, geo, unused);
  for (int i = 0; i < 9; i++)                          // (a singular direction has no point-to-index matrix)
    if (!std::isfinite(geo.p2i[i])) return fail(c, CUBERILLE_ERR_ARGUMENT, name + "direction has no inverse");
  // CUBERILLE_MEM_HOST: a copy of the library's own, complete on return.  The new copy is allocated and filled BEFORE the
  // earlier one is given up, and the setting changes only once nothing can fail any more: a call that fails leaves the
  // context exactly as it was -- off, or on with the earlier image -- and holds no memory of its own.  (One plain copy on
  // the context's stream, whatever the size: the chunk pipeline of cuberille_extract_host is not used here.)
  DevBuf fresh;
  if (location == CUBERILLE_MEM_HOST) {
    const size_t bytes = (size_t)img->dims[0] * (size_t)img->dims[1] * (size_t)img->dims[2] * pixel_size(img->pixel_type);
    (void)hipSetDevice(c->device);
    hipError_t e = fresh.reserve(bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(fresh.p, voxels, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      fresh.release();
      return fail(c, CUBERILLE_ERR_HIP, name + "copy could not be made (" + hipGetErrorString(e) + "): the setting stays as it was");
    }
  }
  // (the earlier copy goes behind whatever may still be reading it; a failure here has released nothing)
  if (const int rc = point_scalars_release(c, false)) { fresh.release(); return rc; }
  ps.copy = fresh;
  ps.vox = location == CUBERILLE_MEM_HOST ? (const void *)ps.copy.p : voxels;
  ps.pixel_type = img->pixel_type;
  for (int i = 0; i < 3; i++) ps.n[i] = (int)img->dims[i];
  ps.geo = geo;
  ps.outside = outside_value;
  ps.on = true;
  return CUBERILLE_OK;
}

static int point_scalars_preconditions(cuberille_ctx *c) {
  if (!c->haveMesh) return fail(c, CUBERILLE_ERR_STATE, "no mesh: call cuberille_extract_* or cuberille_emit first");
  if (!c->ps.have)
    return fail(c, CUBERILLE_ERR_STATE, std::string("no ") + kPointScalarsNoun + ": the last extraction ran with the setting off (" + kPointScalarsFn + ")");
  return CUBERILLE_OK;
}

int cuberille_point_scalars_device(cuberille_ctx *c, const double **d_scalars) {
  if (!c || !d_scalars) return CUBERILLE_ERR_ARGUMENT;
  *d_scalars = nullptr;
  if (const int rc = point_scalars_preconditions(c)) return rc;
  *d_scalars = c->res.n_points ? (const double *)c->ps.rows.row.p : nullptr;   // (a row sized by an earlier mesh is no value of an empty one)
  return CUBERILLE_OK;
}

int cuberille_point_scalars_download(cuberille_ctx *c, double *out, size_t capacity_bytes) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (const int rc = point_scalars_preconditions(c)) return rc;
  const size_t bytes = point_scalars_bytes(c->res.n_points);
  if (capacity_bytes < bytes)
    return fail(c, CUBERILLE_ERR_ARGUMENT, std::string("the ") + kPointScalarsNoun + " take " + std::to_string(bytes) + " bytes, the buffer holds " +
                                           std::to_string(capacity_bytes));
  if (!bytes) return CUBERILLE_OK;
  if (!out) return fail(c, CUBERILLE_ERR_ARGUMENT, "null output pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  return download_pipelined(c, out, c->ps.rows.row.p, bytes);
}

int cuberille_set_cell_pixels(cuberille_ctx *c, int on) { return set_attr(c, ATTR_CELL_PIXELS, on); }

int cuberille_cell_pixels_device(cuberille_ctx *c, const void **d_pixels, int *pixel_type) {
  if (!c || !d_pixels) return CUBERILLE_ERR_ARGUMENT;
  *d_pixels = nullptr;
  if (const int rc = attr_preconditions(c, ATTR_CELL_PIXELS)) return rc;
  *d_pixels = c->res.n_cells ? c->row(ROW_CELL_PIX).p : nullptr;   // (a row sized by an earlier mesh is no value of an empty one)
  if (pixel_type) *pixel_type = c->pixel_type;
  return CUBERILLE_OK;
}

int cuberille_cell_pixels_download(cuberille_ctx *c, void *out, size_t capacity_bytes) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (const int rc = attr_preconditions(c, ATTR_CELL_PIXELS)) return rc;
  const size_t bytes = mesh_row_bytes(c, ROW_CELL_PIX);
  if (capacity_bytes < bytes)
    return fail(c, CUBERILLE_ERR_ARGUMENT, "the cell pixels take " + std::to_string(bytes) + " bytes, the buffer holds " + std::to_string(capacity_bytes));
  if (!bytes) return CUBERILLE_OK;
  if (!out) return fail(c, CUBERILLE_ERR_ARGUMENT, "null output pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  return download_pipelined(c, out, c->row(ROW_CELL_PIX).p, bytes);
}

int cuberille_set_components(cuberille_ctx *c, int on) {
  bool released = false;
  if (const int rc = set_attr(c, ATTR_COMPONENTS, on, &released)) return rc;
  if (!released) return CUBERILLE_OK;
  c->nComponents = 0;
  // (... and the other rows' spares, which cuberille_keep_components reserved.  Where a kept mesh lives in a row sized by the kept
  //  counts, it moves back into the buffer the extraction was sized for -- one copy of the kept size -- so that the context holds
  //  the buffers it held before the setting was on, and the next extraction reserves nothing again)
  if (c->haveMesh) {
    for (int r = 0; r < N_ROWS; r++) {
      MeshRow &m = c->rows[r];
      const int a = kRows[r].attr;
      if (a == ATTR_COMPONENTS || m.spare.cap <= m.row.cap || !m.row.p) continue;
      const size_t bytes = a == ATTR_NONE || c->attr[a].have ? mesh_row_bytes(c, r) : 0;
      if (bytes) HIP_TRY(c, hipMemcpyAsync(m.spare.p, m.row.p, bytes, hipMemcpyDeviceToDevice, c->stream));
      std::swap(m.row, m.spare);
    }
    if (MeshRow &m = c->ps.rows; m.spare.cap > m.row.cap && m.row.p) {      // (the point scalars' pair, beside the table)
      const size_t bytes = c->ps.have ? point_scalars_bytes(c->res.n_points) : 0;
      if (bytes) HIP_TRY(c, hipMemcpyAsync(m.spare.p, m.row.p, bytes, hipMemcpyDeviceToDevice, c->stream));
      std::swap(m.row, m.spare);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->w.points = (float *)c->row(ROW_POINTS).p;
    c->w.cells = (u64 *)c->row(ROW_CELLS).p;
  }
  for (MeshRow &m : c->rows) m.spare.release();
  c->ps.rows.spare.release();
  return CUBERILLE_OK;
}

int cuberille_components_info(cuberille_ctx *c, uint64_t *n_components) {
  if (!c || !n_components) return CUBERILLE_ERR_ARGUMENT;
  *n_components = 0;
  if (const int rc = attr_preconditions(c, ATTR_COMPONENTS)) return rc;
  *n_components = c->nComponents;
  return CUBERILLE_OK;
}

int cuberille_components_device(cuberille_ctx *c, const uint32_t **d_point_component, const uint32_t **d_cell_component,
                                const uint64_t **d_component_cells) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (d_point_component) *d_point_component = nullptr;
  if (d_cell_component) *d_cell_component = nullptr;
  if (d_component_cells) *d_component_cells = nullptr;
  if (const int rc = attr_preconditions(c, ATTR_COMPONENTS)) return rc;
  // (rows sized by an earlier mesh are no values of an empty one)
  if (d_point_component && c->res.n_points) *d_point_component = (const uint32_t *)c->row(ROW_COMP_POINT).p;
  if (d_cell_component && c->res.n_cells) *d_cell_component = (const uint32_t *)c->row(ROW_COMP_CELL).p;
  if (d_component_cells && c->nComponents) *d_component_cells = (const uint64_t *)c->row(ROW_COMP_COUNT).p;
  return CUBERILLE_OK;
}

int cuberille_components_download(cuberille_ctx *c, uint32_t *point_component, uint32_t *cell_component, uint64_t *component_cells,
                                  size_t capacity_components) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (const int rc = attr_preconditions(c, ATTR_COMPONENTS)) return rc;
  if (component_cells && capacity_components < c->nComponents)
    return fail(c, CUBERILLE_ERR_ARGUMENT, "the mesh has " + std::to_string(c->nComponents) + " components, the buffer holds " +
                                           std::to_string(capacity_components));
  HIP_TRY(c, hipSetDevice(c->device));
  if (point_component && c->res.n_points)
    if (const int rc = download_pipelined(c, point_component, c->row(ROW_COMP_POINT).p, mesh_row_bytes(c, ROW_COMP_POINT))) return rc;
  if (cell_component && c->res.n_cells)
    if (const int rc = download_pipelined(c, cell_component, c->row(ROW_COMP_CELL).p, mesh_row_bytes(c, ROW_COMP_CELL))) return rc;
  if (component_cells && c->nComponents)
    if (const int rc = download_pipelined(c, component_cells, c->row(ROW_COMP_COUNT).p, mesh_row_bytes(c, ROW_COMP_COUNT))) return rc;
  return CUBERILLE_OK;
}

int cuberille_keep_components(cuberille_ctx *c, int rule, uint64_t n, const uint8_t *host_mask, size_t mask_len,
                              uint64_t *n_points, uint64_t *n_cells, uint64_t *n_components, float *ms) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (rule != CUBERILLE_KEEP_LARGEST && rule != CUBERILLE_KEEP_MIN_CELLS && rule != CUBERILLE_KEEP_MASK)
    return fail(c, CUBERILLE_ERR_ARGUMENT, "cuberille_keep_components: unknown rule " + std::to_string(rule));
  if (c->stepMode != 0)
    return fail(c, CUBERILLE_ERR_STATE, "cuberille_keep_components: a step is open on this context, its mesh and components are not complete");
  if (!c->haveMesh)
    return fail(c, CUBERILLE_ERR_STATE, "cuberille_keep_components: no mesh, so no components: call cuberille_extract_* or cuberille_emit first");
  if (c->slabMode)
    return fail(c, CUBERILLE_ERR_STATE, "cuberille_keep_components: a slab's mesh has no components (a component does not stop at a slab's face)");
  if (!c->attr[ATTR_COMPONENTS].have) return fail(c, CUBERILLE_ERR_STATE, "cuberille_keep_components: " + attr_missing(ATTR_COMPONENTS));
  const u64 K = c->nComponents, nP = c->res.n_points, nC = c->res.n_cells;
  if (rule == CUBERILLE_KEEP_MASK) {
    if (mask_len != K)
      return fail(c, CUBERILLE_ERR_ARGUMENT, "cuberille_keep_components: the mesh has " + std::to_string(K) + " components, the mask " +
                                             std::to_string(mask_len) + " bytes");
    if (K && !host_mask) return fail(c, CUBERILLE_ERR_ARGUMENT, "cuberille_keep_components: null mask");
  }
  // (the cells' positions are 32-bit sums like the labels)
  if (nC >= 0x100000000ULL)
    return fail(c, CUBERILLE_ERR_LIMIT, "cuberille_keep_components: cell positions are 32-bit: not offered with 2^32 cells or more");
  auto report = [&]() {
    if (n_points) *n_points = c->res.n_points;
    if (n_cells) *n_cells = c->res.n_cells;
    if (n_components) *n_components = c->nComponents;
  };
  if (ms) *ms = 0.0f;
  if (!K || !nP) { report(); return CUBERILLE_OK; }          // an empty mesh: all of nothing is kept
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (!c->hostKeep) HIP_TRY(c, hipHostMalloc((void **)&c->hostKeep, 3 * sizeof(u64), hipHostMallocDefault));
  for (int i = 0; i < 2; i++)
    if (!c->keepEv[i]) HIP_TRY(c, hipEventCreate(&c->keepEv[i]));
  // decide and number: keep[K], new_number[K], the mask's bytes; the three totals ahead of the scans' levels
  HIP_TRY(c, c->keepSel.reserve((size_t)K * (2 * sizeof(u32) + 1)));
  HIP_TRY(c, c->keepScan.reserve(keep_scan_bytes(K, nP, nC)));
  KeepRows k{};
  k.keep = (u32 *)c->keepSel.p;
  k.number = k.keep + K;
  k.mask = (const uint8_t *)(k.number + K);
  k.totals = (u64 *)c->keepScan.p;
  k.scanK = (u32 *)(k.totals + 3);
  k.scanP = k.scanK + comp_scan_plan(K).entries;
  k.scanC = k.scanP + comp_scan_plan(nP).entries;
  const CompRows r = comp_rows(c);
  HIP_TRY(c, hipEventRecord(c->keepEv[0], s));
  if (rule == CUBERILLE_KEEP_MASK)
    HIP_TRY(c, hipMemcpyAsync((void *)k.mask, host_mask, (size_t)K, hipMemcpyHostToDevice, s));
  HIP_TRY(c, launch_keep_count(c->w, r, k, rule, n, K, nP, nC, s));
  HIP_TRY(c, hipMemcpyAsync(c->hostKeep, k.totals, 3 * sizeof(u64), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));                       // the one read: K', n_points', n_cells'
  const u64 K2 = c->hostKeep[0], nP2 = c->hostKeep[1], nC2 = c->hostKeep[2];
  if (K2 > K || nP2 > nP || nC2 > nC) return fail(c, CUBERILLE_ERR_STATE, "internal: cuberille_keep_components kept more than there is");
  // (the rows of the mesh that are kept: its own, and those of the attributes it came with)
  bool kept[N_ROWS];
  for (int i = 0; i < N_ROWS; i++) kept[i] = kRows[i].attr == ATTR_NONE || c->attr[kRows[i].attr].have;
  if (K2 != K && K2 != 0) {
    // decided: the spare rows by the kept counts, every one of them before the first scatter (a failure leaves the mesh as it is)
    const size_t pix = pixel_size(c->pixel_type);
    const u64 n2[N_PERS] = {nP2, nC2, K2};
    void *in[N_ROWS] = {}, *out[N_ROWS] = {};                // (null where the mesh has no such row)
    for (int i = 0; i < N_ROWS; i++) {
      if (!kept[i]) continue;
      HIP_TRY(c, c->rows[i].spare.reserve(row_reserve_bytes(i, n2, c->res.verts_per_cell, pix)));
      in[i] = c->rows[i].row.p; out[i] = c->rows[i].spare.p;
    }
    if (c->ps.have) HIP_TRY(c, c->ps.rows.spare.reserve(point_scalars_bytes(nP2)));   // (the point scalars' spare, beside the table)
    const KeepOut o = {(float *)out[ROW_POINTS], (float *)out[ROW_NORMALS], (u64 *)out[ROW_CELLS], out[ROW_CELL_PIX],
                       (u32 *)out[ROW_COMP_POINT], (u32 *)out[ROW_COMP_CELL], (u64 *)out[ROW_COMP_COUNT]};
    Workspace w = c->w;
    w.points = (float *)in[ROW_POINTS];
    w.cells = (u64 *)in[ROW_CELLS];
    HIP_TRY(c, launch_keep_scatter(w, r, k, o, (const float *)in[ROW_NORMALS], in[ROW_CELL_PIX], kept[ROW_CELL_PIX] ? (int)pix : 0,
                                   c->prm.triangles, c->pointOffset, K, nP, nC, s));
    if (c->ps.have)
      HIP_TRY(c, launch_keep_scatter_point_scalars(r, k, (const double *)c->ps.rows.row.p, (double *)c->ps.rows.spare.p, K, nP, s));
  }
  HIP_TRY(c, hipEventRecord(c->keepEv[1], s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (ms) HIP_TRY(c, hipEventElapsedTime(ms, c->keepEv[0], c->keepEv[1]));
  if (K2 != K) {
    if (K2) {
      // the kept mesh is complete in the spare rows: the buffers change places (the earlier ones are the next call's spare rows)
      for (int i = 0; i < N_ROWS; i++)
        if (kept[i]) std::swap(c->rows[i].row, c->rows[i].spare);
      if (c->ps.have) std::swap(c->ps.rows.row, c->ps.rows.spare);
      c->w.points = (float *)c->row(ROW_POINTS).p;
      c->w.cells = (u64 *)c->row(ROW_CELLS).p;
    }
    // (the walk counters, the ms_* fields, the count's tables and the sizes of the next blind launch stay the extraction's)
    c->res.n_points = nP2;
    c->res.n_cells = nC2;
    c->nComponents = K2;
    c->hostMeshValid = false;
  }
  report();
  return CUBERILLE_OK;
}

int cuberille_debug_device_bytes(cuberille_ctx *c, size_t *bytes) {
  if (!c || !bytes) return CUBERILLE_ERR_ARGUMENT;
  *bytes = 0;
  for (const DevBuf *b : device_buffers(c)) *bytes += b->cap;
  return CUBERILLE_OK;
}

int cuberille_hold_gradient(cuberille_ctx *c, int hold) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (c->stepMode != 0) return fail(c, CUBERILLE_ERR_STATE, "a step is open on this context");
  if (!hold || !c->holdGradient) c->heldStep = -1.0;       // (asked again while holding: the same filter object goes on)
  c->holdGradient = hold != 0;
  if (!hold && c->held.img) {
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));     // (a walk may still be reading it)
    c->heldGrad.release();
    c->held = HeldGradient{};
  }
  return CUBERILLE_OK;
}

int cuberille_gradient_held(cuberille_ctx *c, int64_t dims[3]) {
  if (!c) return 0;
  if (dims) for (int i = 0; i < 3; i++) dims[i] = c->held.img ? c->held.n[i] : 0;
  return c->held.img ? 1 : 0;
}

int cuberille_set_interpolator(cuberille_ctx *c, int kind, int spline_order, int coordinate_bits, int coefficient_bits) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (c->stepMode != 0) return fail(c, CUBERILLE_ERR_STATE, "a step is open on this context");
  if (kind == CUBERILLE_INTERP_LINEAR) {
    c->interp = CUBERILLE_INTERP_LINEAR;
    return CUBERILLE_OK;
  }
  if (kind != CUBERILLE_INTERP_BSPLINE) return fail(c, CUBERILLE_ERR_ARGUMENT, "unknown interpolator kind");
  if (spline_order != 3)
    return fail(c, CUBERILLE_ERR_ARGUMENT, "the device B-spline walk implements spline order 3 (the reference driver's SetSplineOrder(3))");
  if (!((coordinate_bits == 32 && coefficient_bits == 32) || (coordinate_bits == 64 && coefficient_bits == 64)))
    return fail(c, CUBERILLE_ERR_ARGUMENT, "the device B-spline walk implements <float, float> (32, 32) and <double, double> (64, 64)");
  c->interp = CUBERILLE_INTERP_BSPLINE;
  c->bsBits = coordinate_bits;
  return CUBERILLE_OK;
}

int cuberille_set_border(cuberille_ctx *c, int pad_width, double pad_value, int64_t pad_value_int) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (c->stepMode != 0) return fail(c, CUBERILLE_ERR_STATE, "a step is open on this context");
  if (pad_width != 0 && pad_width != 1) return fail(c, CUBERILLE_ERR_ARGUMENT, "the implied border is 0 (off) or 1 voxel wide");
  c->padWidth = pad_width;
  c->padValue = pad_value;
  c->padValueInt = (long long)pad_value_int;
  return CUBERILLE_OK;
}

int cuberille_band_check(int pixel_type, const double v[4], const int64_t vi[4]) {
  const char *why = "";
  const int rc = band_check(pixel_type, v, vi, &why);
  if (rc) g_create_error = why;     // (no context to keep the text: cuberille_last_error(NULL), per thread like a failed create's)
  return rc;
}

int cuberille_set_band(cuberille_ctx *c, int on, const double v[4], const int64_t vi[4]) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (c->stepMode != 0) return fail(c, CUBERILLE_ERR_STATE, "a step is open on this context");
  if (!on) {
    c->bandOn = false;
    for (int k = 0; k < 4; k++) { c->bandV[k] = 0.0; c->bandVi[k] = 0; }
    return CUBERILLE_OK;
  }
  if (!v || !vi) return fail(c, CUBERILLE_ERR_ARGUMENT, "a band (cuberille_set_band) needs its four values both ways");
  // (what can be said without the pixel type; the rest at the extraction, by the same validator)
  if (v[0] != v[0] || v[1] != v[1]) return fail(c, CUBERILLE_ERR_ARGUMENT, "band (cuberille_set_band): a bound is NaN");
  c->bandOn = true;
  for (int k = 0; k < 4; k++) { c->bandV[k] = v[k]; c->bandVi[k] = (long long)vi[k]; }
  return CUBERILLE_OK;
}

int cuberille_set_region(cuberille_ctx *c, const int64_t start[3], const int64_t size[3]) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (c->stepMode != 0) return fail(c, CUBERILLE_ERR_STATE, "a step is open on this context");
  if ((start == nullptr) != (size == nullptr)) return fail(c, CUBERILLE_ERR_ARGUMENT, "a region needs both its start and its size");
  if (!size || (size[0] == 0 && size[1] == 0 && size[2] == 0)) {
    c->regionOn = false;
    for (int i = 0; i < 3; i++) c->regionStart[i] = c->regionSize[i] = 0;
    return CUBERILLE_OK;
  }
  // (what can be said without the buffer's dims; the rest at the extraction, by the same validator)
  cuberille_image_desc any{}, box;
  for (int i = 0; i < 3; i++) any.dims[i] = 0x7fffffffLL;
  const char *why = "";
  const int rc = region_check(&any, start, size, &box, &why);
  if (rc == CUBERILLE_ERR_ARGUMENT) return fail(c, rc, why);
  c->regionOn = true;
  for (int i = 0; i < 3; i++) { c->regionStart[i] = start[i]; c->regionSize[i] = size[i]; }
  return CUBERILLE_OK;
}

int cuberille_bspline_coefficients_info(cuberille_ctx *c, int64_t dims[3], int *coefficient_bits) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (dims) for (int i = 0; i < 3; i++) dims[i] = c->bsValidBits ? c->bsDims[i] : 0;
  if (coefficient_bits) *coefficient_bits = c->bsValidBits;
  return c->bsValidBits ? 1 : 0;
}

int cuberille_bspline_coefficients(cuberille_ctx *c, void *host_out, size_t capacity_bytes) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  if (!c->bsValidBits) return fail(c, CUBERILLE_ERR_STATE, "no B-spline extraction on this context has projected a vertex");
  const size_t bytes = (size_t)c->bsDims[0] * (size_t)c->bsDims[1] * (size_t)c->bsDims[2] * (size_t)(c->bsValidBits / 8);
  if (!host_out || capacity_bytes < bytes) return fail(c, CUBERILLE_ERR_ARGUMENT, "the output buffer is smaller than the coefficient image");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(host_out, c->bsCoef.p, bytes, hipMemcpyDeviceToHost));
  return CUBERILLE_OK;
}

int cuberille_release_host_mesh(cuberille_ctx *c) {
  if (!c) return CUBERILLE_ERR_ARGUMENT;
  c->hostPoints.release();
  c->hostCells.release();
  c->hostMeshValid = false;
  return CUBERILLE_OK;
}

int cuberille_mesh_write_vtk(cuberille_ctx *c, const char *path, int n_threads) {
  if (!c || !path) return CUBERILLE_ERR_ARGUMENT;
  if (!c->haveMesh) return fail(c, CUBERILLE_ERR_STATE, "no mesh: call cuberille_extract_* or cuberille_emit first");
  if (c->slabMesh) return fail(c, CUBERILLE_ERR_STATE, "a slab mesh is not self-contained: concatenate the rank buffers and call cuberille_write_vtk_buffers");
  const cuberille_result &r = c->res;
  float *pts = nullptr;
  uint64_t *cells = nullptr;
  const int rc = cuberille_mesh_host(c, &pts, &cells);
  if (rc != CUBERILLE_OK) return rc;
  int wr = cuberille_write_vtk_buffers(path, pts, r.n_points, cells, r.n_cells, r.verts_per_cell, n_threads);
  const bool withNormals = c->attr[ATTR_NORMALS].have, withPixels = c->attr[ATTR_CELL_PIXELS].have, withComponents = c->attr[ATTR_COMPONENTS].have;
  if (wr == CUBERILLE_OK && withNormals) {
    // a context that holds normals: POINT_DATA n / NORMALS normals float behind the polygons (setting off: the file as it always was)
    std::vector<float> nrm(mesh_row_bytes(c, ROW_NORMALS) / sizeof(float));
    const int dl = cuberille_normals_download(c, nrm.data());
    if (dl != CUBERILLE_OK) return dl;
    wr = cuberille::append_vtk_normals(path, nrm.data(), r.n_points, n_threads);
  }
  // a context that holds components: SCALARS component unsigned_int 1 in POINT_DATA (behind the normals) and in CELL_DATA (behind
  // the cell pixels), either block opened here where nothing else has (setting off: the file as it was)
  std::vector<uint32_t> pointComp, cellComp;
  if (wr == CUBERILLE_OK && withComponents) {
    pointComp.resize(mesh_row_bytes(c, ROW_COMP_POINT) / sizeof(uint32_t));
    cellComp.resize(mesh_row_bytes(c, ROW_COMP_CELL) / sizeof(uint32_t));
    const int dl = cuberille_components_download(c, pointComp.data(), cellComp.data(), nullptr, 0);
    if (dl != CUBERILLE_OK) return dl;
    wr = cuberille::append_vtk_components(path, withNormals ? nullptr : "POINT_DATA", pointComp.data(), r.n_points);
  }
  if (wr == CUBERILLE_OK && c->ps.have) {
    // a context that holds point scalars: SCALARS point_scalar double 1, last in POINT_DATA (setting off: the file as it was)
    std::vector<double> val(r.n_points);
    const int dl = cuberille_point_scalars_download(c, val.data(), val.size() * sizeof(double));
    if (dl != CUBERILLE_OK) return dl;
    wr = cuberille::append_vtk_point_scalars(path, withNormals || withComponents ? nullptr : "POINT_DATA", val.data(), r.n_points);
  }
  if (wr == CUBERILLE_OK && withPixels) {
    // a context that holds cell pixels: CELL_DATA n / SCALARS pixel <type> 1 behind everything else (setting off: the file as it was)
    std::vector<char> pix(mesh_row_bytes(c, ROW_CELL_PIX));
    const int dl = cuberille_cell_pixels_download(c, pix.data(), pix.size());
    if (dl != CUBERILLE_OK) return dl;
    wr = cuberille::append_vtk_cell_pixels(path, pix.data(), c->pixel_type, r.n_cells);
  }
  if (wr == CUBERILLE_OK && withComponents)
    wr = cuberille::append_vtk_components(path, withPixels ? nullptr : "CELL_DATA", cellComp.data(), r.n_cells);
  if (wr != CUBERILLE_OK) return fail(c, wr, std::string("cannot write ") + path);
  return CUBERILLE_OK;
}

int cuberille_debug_bits(cuberille_ctx *c, uint64_t *words, size_t n_words) {
  if (!c || !words) return CUBERILLE_ERR_ARGUMENT;
  if (!c->counted && !c->haveMesh) return fail(c, CUBERILLE_ERR_STATE, "no classified volume on this context");
  const size_t have = (size_t)c->g.ny * c->g.nzb * c->g.W;
  if (n_words > have) return fail(c, CUBERILLE_ERR_ARGUMENT, "more words requested than the bit volume holds");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(words, c->bits.p, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CUBERILLE_OK;
}

int cuberille_slice_occupancy(cuberille_ctx *c, uint32_t *occupied, size_t n_slices) {
  if (!c || !occupied) return CUBERILLE_ERR_ARGUMENT;
  if (!c->counted && !c->haveMesh) return fail(c, CUBERILLE_ERR_STATE, "no classified volume on this context");
  if (n_slices > (size_t)c->g.nzb) return fail(c, CUBERILLE_ERR_ARGUMENT, "more slices requested than the buffer holds");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(occupied, c->w.sliceOcc, n_slices * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CUBERILLE_OK;
}

}  // extern "C"

// ---- cuberille_group: N contexts, one host-resident volume, one mesh ------------------------------------------------------
// Every member uploads its slab plus the full halo straight from the caller's image on its own stream and link, so no
// member needs another's voxels.  The host sums the counts, plans quirk Q1's hand-overs (distributed.alias_plan, restated)
// and stages them through host memory, so the same code runs whether the members share a device or not.

struct cuberille_group {
  std::vector<cuberille_ctx *> ctx;
  std::string err;
  int used = 0;                          // members the last extraction cut the volume for (min(n, Nz))
  std::vector<cuberille_result> slabRes; // ... and each one's result
  std::vector<u64> pointOff, cellOff;    // ... its first point and first cell in the assembled mesh
  cuberille_result res{};
  bool haveMesh = false;
  HostBuf hostPoints, hostCells;         // cuberille_group_mesh_host: the assembled mesh
  bool hostMeshValid = false;
  int drillSlab = -1;                    // cuberille_group_debug_fail_alloc: armed for the next extraction's upload and count
  long long drillAt = -1;
};

namespace {

constexpr int kGroupMax = 64;

int gfail(cuberille_group *g, int code, const std::string &msg) {
  g->err = msg;
  return code;
}

// The cuts of a group of n: slabs of equal thickness (distributed.slab_range), each buffer the owned range widened by the
// full required halo and clipped to the volume.  bounds[4 i ..]: own_z0, own_z1, buf_z0, buf_z1.
int group_plan_impl(const cuberille_image_desc *img, const cuberille_params *prm, int n, int64_t *bounds, int *n_used,
                    std::string *why) {
  auto no = [why](const char *m) { if (why) *why = m; return CUBERILLE_ERR_ARGUMENT; };
  if (!img || !prm) return no("null image or parameter pointer");
  if (n < 1 || n > kGroupMax) return no("a group has 1 to 64 members");
  for (int i = 0; i < 3; i++) {
    if (img->dims[i] < 1) return no("image dimensions must be >= 1");
    if (!(img->spacing[i] > 0.0)) return no("spacing must be > 0");
  }
  if (prm->project_vertices && prm->gradient_variant == CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN)
    return no("the recursive-Gaussian gradient filters whole lines of the volume: not offered on slabs, so not in a group");
  int64_t below = 0, above = 0;
  if (cuberille_required_halo(img, prm, &below, &above) != CUBERILLE_OK) return no("bad image description or parameters");
  const int64_t nz = img->dims[2];
  const int used = (int64_t)n < nz ? n : (int)nz;
  const int64_t base = nz / used, rem = nz % used;
  for (int r = 0; r < used; r++) {
    const int64_t z0 = r * base + (r < rem ? r : rem), z1 = z0 + base + (r < rem ? 1 : 0);
    if (bounds) {
      bounds[4 * r] = z0;
      bounds[4 * r + 1] = z1;
      bounds[4 * r + 2] = z0 - below > 0 ? z0 - below : 0;
      bounds[4 * r + 3] = z1 + above < nz ? z1 + above : nz;
    }
  }
  if (n_used) *n_used = used;
  return CUBERILLE_OK;
}

// Let every member's streams finish (a failure on one slab: the others may still be copying from the caller's image).
void group_drain(cuberille_group *g) {
  for (cuberille_ctx *c : g->ctx) {
    if (hipSetDevice(c->device) != hipSuccess) continue;
    (void)hipStreamSynchronize(c->stream);
    if (c->copyStream) (void)hipStreamSynchronize(c->copyStream);
    (void)hipGetLastError();
  }
}

// One slab's outcome of a phase: the call that failed and the member's text
struct SlabStatus {
  int rc = CUBERILLE_OK;
  std::string what;
  void set(int code, const char *call, cuberille_ctx *c) {
    rc = code;
    what = std::string(call) + ": " + (c ? c->err : std::string());
  }
};

// Run f(i) for i in [0, n) on threads of their own (one per slab), f(0) on the calling thread.
template <class F> void for_each_slab(int n, F f) {
  std::vector<std::thread> th;
  for (int i = 1; i < n; i++) th.emplace_back([&f, i] { f(i); });
  if (n > 0) f(0);
  for (auto &t : th) t.join();
}

// The first failed slab as the group's error (after draining every member), or OK
int group_failure(cuberille_group *g, const std::vector<SlabStatus> &st) {
  for (size_t i = 0; i < st.size(); i++)
    if (st[i].rc != CUBERILLE_OK) {
      group_drain(g);
      return gfail(g, st[i].rc, "slab " + std::to_string(i) + ": " + st[i].what);
    }
  return CUBERILLE_OK;
}

// One entry of quirk Q1's hand-over plan: consumer slab, source slab, source slice, whether the consumer needs the plane
struct AliasEntry { int consumer, source; int64_t zp; bool plane; };

}  // namespace

extern "C" {

int cuberille_group_create(cuberille_group **out, const int *device_ids, int n) {
  if (!out) return fail(nullptr, CUBERILLE_ERR_ARGUMENT, "null output pointer");
  *out = nullptr;
  if (!device_ids || n < 1 || n > kGroupMax) return fail(nullptr, CUBERILLE_ERR_ARGUMENT, "a group has 1 to 64 members");
  cuberille_group *g = new (std::nothrow) cuberille_group;
  if (!g) return fail(nullptr, CUBERILLE_ERR_ARGUMENT, "out of host memory");
  for (int i = 0; i < n; i++) {
    cuberille_ctx *c = nullptr;
    const int rc = cuberille_create(&c, device_ids[i]);
    if (rc != CUBERILLE_OK) {
      const std::string why = g_create_error;
      cuberille_group_destroy(g);
      return fail(nullptr, rc, "member " + std::to_string(i) + " (device " + std::to_string(device_ids[i]) + "): " + why);
    }
    g->ctx.push_back(c);
  }
  *out = g;
  return CUBERILLE_OK;
}

void cuberille_group_destroy(cuberille_group *g) {
  if (!g) return;
  for (cuberille_ctx *c : g->ctx) cuberille_destroy(c);
  g->hostPoints.release();
  g->hostCells.release();
  delete g;
}

const char *cuberille_group_last_error(const cuberille_group *g) { return g ? g->err.c_str() : g_create_error.c_str(); }

cuberille_ctx *cuberille_group_context(cuberille_group *g, int i) {
  if (!g || i < 0 || i >= (int)g->ctx.size()) return nullptr;
  return g->ctx[(size_t)i];
}

int cuberille_group_plan(const cuberille_image_desc *img, const cuberille_params *prm, int n, int64_t *bounds, int *n_used) {
  return group_plan_impl(img, prm, n, bounds, n_used, nullptr);
}

int cuberille_group_warm_up(cuberille_group *g, const cuberille_image_desc *img, const cuberille_params *prm) {
  if (!g) return CUBERILLE_ERR_ARGUMENT;
  const int n = (int)g->ctx.size();
  std::vector<int64_t> b(4 * (size_t)n);
  int used = 0;
  cuberille_params dflt{};
  dflt.generate_triangles = 1; dflt.project_vertices = 1; dflt.distance_threshold = 0.5; dflt.step_length = -1.0;
  dflt.relaxation = 0.95; dflt.max_steps = 50; dflt.emulate_empty_slice_aliasing = 1;
  if (img) {
    std::string why;
    if (group_plan_impl(img, prm ? prm : &dflt, n, b.data(), &used, &why) != CUBERILLE_OK)
      return gfail(g, CUBERILLE_ERR_ARGUMENT, "cuberille_group_warm_up: " + why);
  }
  const int share = std::max(1, pool_threads_default() / std::max(1, used ? used : n));
  std::vector<SlabStatus> st((size_t)n);
  for_each_slab(n, [&](int i) {
    cuberille_ctx *c = g->ctx[(size_t)i];
    c->poolThreads = share;
    int rc;
    if (i < used) {
      cuberille_image_desc d = *img;
      d.dims[2] = b[4 * (size_t)i + 3] - b[4 * (size_t)i + 2];
      rc = cuberille_warm_up(c, &d, prm);
    } else {
      rc = cuberille_warm_up(c, nullptr, nullptr);
    }
    if (rc) st[(size_t)i].set(rc, "cuberille_warm_up", c);
  });
  return group_failure(g, st);
}

int cuberille_group_debug_fail_alloc(cuberille_group *g, int slab, int64_t n) {
  if (!g || slab < -1 || slab >= (int)g->ctx.size()) return CUBERILLE_ERR_ARGUMENT;
  g->drillSlab = n < 0 ? -1 : slab;
  g->drillAt = n < 0 ? -1 : (long long)n;
  return CUBERILLE_OK;
}

int cuberille_group_extract_host(cuberille_group *g, const cuberille_image_desc *img, const void *host_voxels,
                                 const cuberille_params *prm, cuberille_result *res) {
  if (!g) return CUBERILLE_ERR_ARGUMENT;
  g->haveMesh = false;
  g->hostMeshValid = false;
  const int drillSlab = g->drillSlab;
  const long long drillAt = g->drillAt;
  g->drillSlab = -1;                         // (one extraction)
  g->drillAt = -1;
  if (!img || !host_voxels || !prm) return gfail(g, CUBERILLE_ERR_ARGUMENT, "null image, voxel or parameter pointer");
  const int n = (int)g->ctx.size();
  std::vector<int64_t> b(4 * (size_t)n);
  int used = 0;
  std::string why;
  if (group_plan_impl(img, prm, n, b.data(), &used, &why) != CUBERILLE_OK) return gfail(g, CUBERILLE_ERR_ARGUMENT, why);
  for (int i = 0; i < n; i++) {
    const cuberille_ctx *c = g->ctx[(size_t)i];
    View view;
    const char *why = "";
    const int vrc = resolve_view(c, img, projection_features(prm), ROUTE_GROUP, &view, &why);
    if (vrc) return gfail(g, vrc, "member " + std::to_string(i) + " " + why);
    if (c->interp == CUBERILLE_INTERP_BSPLINE)
      return gfail(g, CUBERILLE_ERR_ARGUMENT, "member " + std::to_string(i) + " has the B-spline interpolator set: its "
                                              "prefilter needs whole lines of the volume, not offered in a group");
    if (c->holdGradient)
      return gfail(g, CUBERILLE_ERR_ARGUMENT, "member " + std::to_string(i) + " holds a gradient (cuberille_hold_gradient): "
                                              "it belongs to a whole volume, not offered in a group");
    if (const int arc = attrs_offered(c, prm, ROUTE_GROUP, nullptr, 0, &why)) return gfail(g, arc, "member " + std::to_string(i) + " " + why);
  }
  {
    const int rc = validate(g->ctx[0], img, host_voxels, prm);
    if (rc) return gfail(g, rc, g->ctx[0]->err);
  }
  const size_t sliceBytes = (size_t)img->dims[0] * img->dims[1] * pixel_size(img->pixel_type);
  const int share = std::max(1, pool_threads_default() / used);   // the staging threads of ONE context, split
  const bool q1 = prm->emulate_empty_slice_aliasing != 0;

  // 1. upload and count, every slab at once; a slab that no other can change starts its vertex phase right away
  std::vector<SlabStatus> st((size_t)used);
  std::vector<uint64_t> np((size_t)used, 0), nc((size_t)used, 0);
  std::vector<cuberille_slab_status> info((size_t)used);
  for_each_slab(used, [&](int i) {
    cuberille_ctx *c = g->ctx[(size_t)i];
    SlabStatus &s = st[(size_t)i];
    const int64_t *bi = &b[4 * (size_t)i];
    c->poolThreads = share;
    cuberille_image_desc d = *img;
    d.dims[2] = bi[3] - bi[2];
    const cuberille_slab slab = {img->dims[2], bi[2], bi[0], bi[1], 0, 0, nullptr, nullptr};
    const size_t bytes = sliceBytes * (size_t)d.dims[2], base = sliceBytes * (size_t)bi[2];
    if (drillSlab == i || (drillSlab == -1 && drillAt >= 0)) g_fail_alloc_countdown = drillAt;
    int rc = CUBERILLE_OK;
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = c->voxOwn.reserve(bytes);
    if (e != hipSuccess) {
      rc = fail(c, CUBERILLE_ERR_HIP, std::string("device copy of the slab: ") + hipGetErrorString(e));
      s.set(rc, "upload", c);
    } else if (upload_in_chunks(sliceBytes, bytes)) {
      rc = validate(c, &d, host_voxels, prm);
      if (!rc) rc = count_host_chunked(c, &d, host_voxels, base, prm, &slab, View{});
      if (!rc) { np[(size_t)i] = c->res.n_points; nc[(size_t)i] = c->res.n_cells; }
      if (rc) s.set(rc, "chunked upload and count", c);
    } else {
      e = hipMemcpyAsync(c->voxOwn.p, (const char *)host_voxels + base, bytes, hipMemcpyHostToDevice, c->stream);
      if (e != hipSuccess) {
        rc = fail(c, CUBERILLE_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
        s.set(rc, "upload", c);
      } else if ((rc = cuberille_count(c, &d, c->voxOwn.p, prm, &slab, &np[(size_t)i], &nc[(size_t)i])) != CUBERILLE_OK) {
        s.set(rc, "cuberille_count", c);
      }
    }
    g_fail_alloc_countdown = -1;
    if (rc) return;
    info[(size_t)i].alias_z = -1;
    if (q1 && (rc = cuberille_slab_info(c, &info[(size_t)i])) != CUBERILLE_OK) { s.set(rc, "cuberille_slab_info", c); return; }
    if (info[(size_t)i].alias_z < 0 && (rc = cuberille_emit_points(c)) != CUBERILLE_OK) s.set(rc, "cuberille_emit_points", c);
  });
  if (const int rc = group_failure(g, st)) return rc;

  // 2. quirk Q1 across the cuts (distributed.alias_plan): the consumer counts again with the source slice's bits at hand
  std::vector<AliasEntry> plan;
  if (q1)
    for (int r = 1; r < used; r++) {
      const int64_t az = info[(size_t)r].alias_z;
      if (az < 0) continue;
      int src = -1;
      int64_t zp = -1;
      for (int s = 0; s < r; s++) {
        const int64_t h = info[(size_t)s].highest_occupied_z < az ? info[(size_t)s].highest_occupied_z
                                                                   : info[(size_t)s].second_highest_occupied_z;
        if (h >= 0 && h < az && h > zp) { src = s; zp = h; }
      }
      if (src >= 0) plan.push_back({r, src, zp, az >= b[4 * (size_t)r]});   // (az below own_z0: the ghost slice, bits only)
    }
  for (const AliasEntry &a : plan) {
    cuberille_ctx *sc = g->ctx[(size_t)a.source], *cc = g->ctx[(size_t)a.consumer];
    std::vector<SlabStatus> st2((size_t)used);
    const uint64_t *dw = nullptr;
    size_t nw = 0;
    int rc = cuberille_slice_bits_device(sc, a.zp, &dw, &nw);
    if (rc) { st2[(size_t)a.source].set(rc, "cuberille_slice_bits_device", sc); return group_failure(g, st2); }
    std::vector<uint64_t> words(nw);
    hipError_t e = hipSetDevice(sc->device);
    if (e == hipSuccess) e = hipMemcpyAsync(words.data(), dw, nw * sizeof(uint64_t), hipMemcpyDeviceToHost, sc->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(sc->stream);
    if (e != hipSuccess) {
      st2[(size_t)a.source].set(fail(sc, CUBERILLE_ERR_HIP, hipGetErrorString(e)), "quirk-Q1 source bits to the host", sc);
      return group_failure(g, st2);
    }
    DevBuf dev;
    e = hipSetDevice(cc->device);
    if (e == hipSuccess) e = dev.reserve(nw * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemcpyAsync(dev.p, words.data(), nw * sizeof(uint64_t), hipMemcpyHostToDevice, cc->stream);
    if (e != hipSuccess) st2[(size_t)a.consumer].set(fail(cc, CUBERILLE_ERR_HIP, hipGetErrorString(e)), "quirk-Q1 source bits to the consumer", cc);
    else if ((rc = cuberille_recount(cc, dev.p, &np[(size_t)a.consumer], &nc[(size_t)a.consumer])) != CUBERILLE_OK)
      st2[(size_t)a.consumer].set(rc, "cuberille_recount", cc);
    dev.release();                           // (the recount has waited for its stream)
    if (const int rc2 = group_failure(g, st2)) return rc2;
  }
  std::vector<u64> poff((size_t)used + 1, 0);
  for (int i = 0; i < used; i++) poff[(size_t)i + 1] = poff[(size_t)i] + np[(size_t)i];

  // 3. emit: the slabs of a hand-over in rank order (the source's plane after its emit, before the consumer's), the rest at once
  std::vector<char> inChain((size_t)used, 0);
  for (const AliasEntry &a : plan)
    if (a.plane) inChain[(size_t)a.consumer] = inChain[(size_t)a.source] = 1;
  const size_t corners = (size_t)(img->dims[0] + 1) * (size_t)(img->dims[1] + 1);
  std::vector<std::vector<uint64_t>> planeIds(plan.size());
  std::vector<std::vector<float>> planePts(plan.size());
  std::vector<SlabStatus> est((size_t)used);
  std::vector<cuberille_result> sres((size_t)used);
  auto emitOne = [&](int i) {
    cuberille_ctx *c = g->ctx[(size_t)i];
    SlabStatus &s = est[(size_t)i];
    DevBuf ids, pts;
    if (hipSetDevice(c->device) != hipSuccess) { s.set(fail(c, CUBERILLE_ERR_HIP, "hipSetDevice"), "cuberille_emit", c); return false; }
    for (size_t k = 0; k < plan.size(); k++) {
      if (!plan[k].plane || plan[k].consumer != i) continue;
      hipError_t e = hipSetDevice(c->device);
      if (e == hipSuccess) e = ids.reserve(corners * sizeof(uint64_t));
      if (e == hipSuccess) e = pts.reserve(corners * 3 * sizeof(float));
      if (e == hipSuccess) e = hipMemcpyAsync(ids.p, planeIds[k].data(), corners * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(pts.p, planePts[k].data(), corners * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
      if (e != hipSuccess) { s.set(fail(c, CUBERILLE_ERR_HIP, hipGetErrorString(e)), "quirk-Q1 plane to the consumer", c); return false; }
      const int rc = cuberille_set_alias_plane(c, (const uint64_t *)ids.p, (const float *)pts.p);
      if (rc) { s.set(rc, "cuberille_set_alias_plane", c); return false; }
    }
    int rc = cuberille_emit(c, poff[(size_t)i], &sres[(size_t)i]);
    ids.release();
    pts.release();
    if (rc) { s.set(rc, "cuberille_emit", c); return false; }
    for (size_t k = 0; k < plan.size(); k++) {
      if (!plan[k].plane || plan[k].source != i) continue;
      planeIds[k].resize(corners);
      planePts[k].resize(corners * 3);
      hipError_t e = hipSetDevice(c->device);
      if (e == hipSuccess) e = ids.reserve(corners * sizeof(uint64_t));
      if (e == hipSuccess) e = pts.reserve(corners * 3 * sizeof(float));
      if (e != hipSuccess) { s.set(fail(c, CUBERILLE_ERR_HIP, hipGetErrorString(e)), "quirk-Q1 plane of the source", c); return false; }
      if ((rc = cuberille_alias_plane_device(c, plan[k].zp, (uint64_t *)ids.p, (float *)pts.p)) != CUBERILLE_OK) {
        s.set(rc, "cuberille_alias_plane_device", c);
        return false;
      }
      e = hipMemcpyAsync(planeIds[k].data(), ids.p, corners * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(planePts[k].data(), pts.p, corners * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) { s.set(fail(c, CUBERILLE_ERR_HIP, hipGetErrorString(e)), "quirk-Q1 plane to the host", c); return false; }
    }
    return true;
  };
  std::vector<int> lanes;                    // -1: the hand-over chain, in rank order, on one thread
  if (std::find(inChain.begin(), inChain.end(), 1) != inChain.end()) lanes.push_back(-1);
  for (int i = 0; i < used; i++) if (!inChain[(size_t)i]) lanes.push_back(i);
  for_each_slab((int)lanes.size(), [&](int l) {
    if (lanes[(size_t)l] >= 0) { (void)emitOne(lanes[(size_t)l]); return; }
    for (int i = 0; i < used; i++)
      if (inChain[(size_t)i] && !emitOne(i)) return;   // (a failed link ends the chain: the later ones need its plane)
  });
  if (const int rc = group_failure(g, est)) return rc;

  // 4. one result: counts and walk statistics summed, device times the largest of the slabs
  cuberille_result r{};
  r.verts_per_cell = prm->generate_triangles ? 3 : 4;
  g->pointOff.assign((size_t)used, 0);
  g->cellOff.assign((size_t)used, 0);
  for (int i = 0; i < used; i++) {
    const cuberille_result &s = sres[(size_t)i];
    g->pointOff[(size_t)i] = r.n_points;
    g->cellOff[(size_t)i] = r.n_cells;
    r.n_points += s.n_points; r.n_cells += s.n_cells;
    r.proj_iterations += s.proj_iterations; r.proj_stop_threshold += s.proj_stop_threshold;
    r.proj_stop_steps += s.proj_stop_steps; r.n_escaped += s.n_escaped;
    float *dst[] = {&r.ms_classify, &r.ms_count, &r.ms_scan, &r.ms_emit_points, &r.ms_project, &r.ms_emit_cells, &r.ms_total, &r.ms_pass};
    const float src[] = {s.ms_classify, s.ms_count, s.ms_scan, s.ms_emit_points, s.ms_project, s.ms_emit_cells, s.ms_total, s.ms_pass};
    for (int k = 0; k < 8; k++) *dst[k] = std::max(*dst[k], src[k]);
  }
  g->slabRes = sres;
  g->used = used;
  g->res = r;
  g->haveMesh = true;
  g->err.clear();
  if (res) *res = r;
  return CUBERILLE_OK;
}

int cuberille_group_slab_result(const cuberille_group *g, int i, cuberille_result *res) {
  if (!g || !res) return CUBERILLE_ERR_ARGUMENT;
  if (!g->haveMesh) return CUBERILLE_ERR_STATE;
  if (i < 0 || i >= g->used) return CUBERILLE_ERR_ARGUMENT;
  *res = g->slabRes[(size_t)i];
  return CUBERILLE_OK;
}

int cuberille_group_mesh_host(cuberille_group *g, float **points, uint64_t **cells) {
  if (!g) return CUBERILLE_ERR_ARGUMENT;
  if (!g->haveMesh) return gfail(g, CUBERILLE_ERR_STATE, "no mesh: call cuberille_group_extract_host first");
  if (!g->hostMeshValid) {
    const cuberille_result &r = g->res;
    const size_t pb = (size_t)r.n_points * 3 * sizeof(float), cb = (size_t)r.n_cells * r.verts_per_cell * sizeof(uint64_t);
    if (!g->hostPoints.reserve(pb ? pb : 1) || !g->hostCells.reserve(cb ? cb : 1))
      return gfail(g, CUBERILLE_ERR_HIP, "cuberille_group_mesh_host: out of host memory");
    // every slab's part into its own range, at once; the staging threads of one context split between them
    std::vector<SlabStatus> st((size_t)g->used);
    const int share = std::max(1, pool_threads_default() / g->used);
    for_each_slab(g->used, [&](int i) {
      cuberille_ctx *c = g->ctx[(size_t)i];
      c->poolThreads = share;
      const int rc = cuberille_mesh_download(c, (float *)g->hostPoints.p + 3 * g->pointOff[(size_t)i],
                                             (uint64_t *)g->hostCells.p + (size_t)r.verts_per_cell * g->cellOff[(size_t)i]);
      if (rc) st[(size_t)i].set(rc, "cuberille_mesh_download", c);
    });
    if (const int rc = group_failure(g, st)) return rc;
    g->hostMeshValid = true;
  }
  if (points) *points = (float *)g->hostPoints.p;
  if (cells) *cells = (uint64_t *)g->hostCells.p;
  return CUBERILLE_OK;
}

int cuberille_group_release_host_mesh(cuberille_group *g) {
  if (!g) return CUBERILLE_ERR_ARGUMENT;
  g->hostPoints.release();
  g->hostCells.release();
  g->hostMeshValid = false;
  return CUBERILLE_OK;
}

int cuberille_group_mesh_write_vtk(cuberille_group *g, const char *path, int n_threads) {
  if (!g || !path) return CUBERILLE_ERR_ARGUMENT;
  float *pts = nullptr;
  uint64_t *cells = nullptr;
  const int rc = cuberille_group_mesh_host(g, &pts, &cells);
  if (rc) return rc;
  const cuberille_result &r = g->res;
  const int wr = cuberille_write_vtk_buffers(path, pts, r.n_points, cells, r.n_cells, r.verts_per_cell, n_threads);
  if (wr != CUBERILLE_OK) return gfail(g, wr, std::string("cannot write ") + path);
  return CUBERILLE_OK;
}

}  // extern "C"
