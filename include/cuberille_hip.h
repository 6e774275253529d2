/*
 * cuberille_hip.h -- C ABI of the MI355X (gfx950) cuberille iso-surface extractor.
 *
 * This is the drop-in boundary of the one accelerated hot path:
 *   itk::CuberilleImageToMeshFilter<TInputImage,TOutputMesh,TInterpolator>::GenerateData()
 *   reference: Source/itkCuberilleImageToMeshFilter.txx:59-216 and everything it calls
 *   (218-332, 439-498; lookup classes Source/itkCuberilleImageToMeshFilter.h:243-313).
 * The C++ filter template of the same name shipped in
 * midas-journal-740_amd/itk/itkCuberilleImageToMeshFilter.h marshals its image and
 * its eight parameters into the structs below inside GenerateData() and fills the
 * itk::Mesh from the flat buffers that come back.  Plain pointers and sizes only:
 * no C++ or torch types cross this line.
 *
 * Library: midas-journal-740_amd/csrc/libcuberille_hip.so (built by
 * __graft_entry__.build() / csrc/Makefile with hipcc --offload-arch=gfx950).
 * There is NO CPU fallback: every entry point that computes returns
 * CUBERILLE_ERR_NO_DEVICE when no gfx950 device is usable.
 *
 * Threading: a context is not thread-safe; distinct contexts are independent and may be
 * created, used and destroyed from different threads at the same time (the text of a failed
 * cuberille_create is kept per thread).  All work is stream-ordered on the context's stream and
 * complete on return unless a function says otherwise.  The library never reads the environment.
 */
#ifndef CUBERILLE_HIP_H
#define CUBERILLE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUBERILLE_ABI_VERSION 13

/* status codes (reference behaviour: the filter has no explicit checks and ITK throws
 * itk::ExceptionObject, Testing/CuberilleTest01.cxx:207-212; the C++ wrapper turns a
 * non-zero status into itkExceptionMacro with cuberille_last_error()) */
enum {
  CUBERILLE_OK = 0,
  CUBERILLE_ERR_ARGUMENT = 1,   /* null pointer, bad pixel type, non-positive size or spacing */
  CUBERILLE_ERR_NO_DEVICE = 2,  /* no usable HIP device / wrong architecture */
  CUBERILLE_ERR_HIP = 3,        /* a HIP runtime call failed; text in cuberille_last_error */
  CUBERILLE_ERR_STATE = 4,      /* call order violated (emit before count, ...) */
  CUBERILLE_ERR_HALO = 5,       /* slab does not carry the halo the owned range needs */
  CUBERILLE_ERR_LIMIT = 6,      /* volume exceeds an implementation limit */
  CUBERILLE_ERR_SOURCE = 7,     /* the chunk source of cuberille_extract_stream reported a failure */
  CUBERILLE_RETRY = 8           /* cuberille_emit_device_offsets only: not an error -- some rank raised a flag (quirk Q1
                                   across slabs, a buffer too small, a walk that left a thin halo); nothing was emitted,
                                   the count stands, continue with the synchronous calls */
};

/* InputPixelType of the filter (h:150: any pixel type the template is instantiated with).  Same numbering as the
 * oracle.  The 64-bit integer types (long / unsigned long / long long on LP64) compare in their own type (txx:139-141)
 * and enter the walk the way ITK's operators take them: through (float) in the gradient taps (I6), through (double)
 * in the interpolation (I5) -- both round to nearest for magnitudes past 2^24 / 2^53. */
enum {
  CUBERILLE_PIX_U8 = 0, CUBERILLE_PIX_I8 = 1, CUBERILLE_PIX_U16 = 2, CUBERILLE_PIX_I16 = 3,
  CUBERILLE_PIX_U32 = 4, CUBERILLE_PIX_I32 = 5, CUBERILLE_PIX_F32 = 6, CUBERILLE_PIX_F64 = 7,
  CUBERILLE_PIX_I64 = 8, CUBERILLE_PIX_U64 = 9
};

/* The input image: replaces itk::Image::{GetBufferedRegion, GetSpacing, GetOrigin,
 * GetDirection, GetBufferPointer} as used at txx:71-99,266-270. */
typedef struct {
  int32_t pixel_type;
  int64_t dims[3];        /* Nx, Ny, Nz of the buffer handed over; x fastest */
  double spacing[3];
  double origin[3];
  double direction[9];    /* row-major direction cosines */
  int64_t index_start[3]; /* GetBufferedRegion().GetIndex(): the ITK index of the buffer's first pixel (0 for an image as read from
                             a file; a cropped or pasted image keeps the index of where it came from).  origin stays the
                             image's GetOrigin() -- the physical position of INDEX 0: TransformIndexToPhysicalPoint (txx:266)
                             and the interpolators (txx:451,455) see position + index_start, as in ITK.  Within +-2^30.
                             (ABI 13; before, a caller moved the origin to the first buffered pixel: the same mesh up to the
                             last bit of a double in the transforms.) */
} cuberille_image_desc;

/* The filter's parameters: h:180-228, constructor defaults txx:33-40. */
typedef struct {
  double iso_value;              /* m_IsoSurfaceValue, an InputPixelType in the reference (h:180-181): converted to the pixel
                                    type like a C cast; outside an integer type's range (or NaN for one): ERR_ARGUMENT */
  int32_t generate_triangles;    /* m_GenerateTriangleFaces (default 1) */
  int32_t project_vertices;      /* m_ProjectVerticesToIsoSurface (default 1) */
  double distance_threshold;     /* m_ProjectVertexSurfaceDistanceThreshold (0.5) */
  double step_length;            /* m_ProjectVertexStepLength (-1 => 0.25*max spacing, txx:82-85; on a context that holds a
                                    gradient, cuberille_hold_gradient: of the FIRST extraction's image, kept like the reference keeps it) */
  double relaxation;             /* m_ProjectVertexStepLengthRelaxationFactor (0.95) */
  uint32_t max_steps;            /* m_ProjectVertexMaximumNumberOfSteps (50) */
  int32_t emulate_empty_slice_aliasing; /* 1: reproduce the two-plane lookup quirk of txx:156-161
                                           when a slice holds no inside voxel */
  int32_t projection_variant;    /* which branch of ProjectVertexToIsoSurface: CUBERILLE_PROJECT_DEFAULT (txx:439-474, what
                                    the reference ships), _ADVANCED (USE_ADVANCED_PROJECTION, txx:340-397) or _LINESEARCH
                                    (USE_LINESEARCH_PROJECTION, txx:398-437) -- the last two are compiled out upstream
                                    (h:22-23); anything else is CUBERILLE_ERR_ARGUMENT */
  int32_t gradient_variant;      /* the gradient image the walk follows: CUBERILLE_GRADIENT_CENTRAL -- itk::GradientImageFilter, what
                                    the reference ships (h:166; txx:478-498) -- or CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN:
                                    USE_GRADIENT_RECURSIVE_GAUSSIAN (h:21,163-164; txx:488-491, compiled out upstream):
                                    itk::GradientRecursiveGaussianImageFilter with sigma = the largest spacing and
                                    NormalizeAcrossScale on.  The reference holds three lines of that; the filter itself is ITK's
                                    (Deriche's recursive Gaussian), restated from its published algorithm: PARITY UNPINNED.  It
                                    needs whole lines, so it is refused on slabs, and at least 4 voxels along every axis */
  int64_t iso_value_int;         /* CUBERILLE_PIX_I64 / _U64 only (iso_value is then ignored): the iso value itself, which a
                                    double cannot hold past 2^53; for _U64 the same 64 bits read as unsigned */
} cuberille_params;

enum { CUBERILLE_PROJECT_DEFAULT = 0, CUBERILLE_PROJECT_ADVANCED = 1, CUBERILLE_PROJECT_LINESEARCH = 2 };
enum { CUBERILLE_GRADIENT_CENTRAL = 0, CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN = 1 };

/* Z-slab placement for multi-GPU runs (one process per GPU).
 * NULL or all-zero ranges mean "the buffer is the whole volume" (the two events are honoured either way: a caller that
 * filled the volume on another stream passes only voxels_ready_event). */
typedef struct {
  int64_t global_nz;        /* Nz of the whole volume */
  int64_t z_begin;          /* global z of the buffer's first slice */
  int64_t own_z0, own_z1;   /* global slices [own_z0, own_z1) this rank emits */
  uint64_t point_id_offset; /* id of this rank's first point (cuberille_extract_device; the two-call form passes it to
                               cuberille_emit after the count all-gather).  Cells need no offset: a cell's id is its
                               position in the rank-ordered concatenation, no buffer holds it */
  uint64_t flags;           /* CUBERILLE_SLAB_* */
  void *halo_ready_event;   /* optional hipEvent_t recorded behind the halo exchange: cuberille_count
                               thresholds the owned slices at once and the halo slices after it */
  void *voxels_ready_event; /* optional hipEvent_t recorded on the stream that produced the OWNED slices:
                               nothing of the buffer is read before it (the context runs on its own stream) */
} cuberille_slab;

/* cuberille_slab::flags.  THIN_HALO: the buffer holds fewer slices around the owned range than the projection walk
 * could reach (cuberille_required_halo) but at least what every vertex needs where it STARTS (cuberille_minimum_halo).
 * A walk that then asks for a slice the buffer lacks (and the volume has) is not clamped: the vertex is put aside,
 * cuberille_result::n_escaped counts it, and cuberille_reproject_escaped walks those vertices again once the caller
 * has the deeper halo -- the neighbours' slices cross the links only when some walk really needed them. */
enum { CUBERILLE_SLAB_THIN_HALO = 1 };

/* What a multi-GPU driver needs to know about the last cuberille_count of a slab besides the counts
 * (it travels in the same all-gather): quirk Q1 re-uses vertices across EMPTY slices, so a rank whose
 * first occupied slice has only empty slices below it, down to the bottom of its buffer, cannot tell
 * whether the reference would alias it to something further down -- the ranks below can. */
typedef struct {
  int32_t alias_source_below_buffer; /* 1: the count assumed "nothing occupied below my buffer"; wrong if a rank
                                        below reports an occupied slice */
  int32_t reserved;
  int64_t lowest_occupied_z;         /* global z of the lowest / highest owned slice holding an inside voxel, -1: none */
  int64_t highest_occupied_z;
  int64_t second_highest_occupied_z; /* the owned occupied slice below highest_occupied_z, -1: none (the source when the
                                        slice the rank above asks about is this rank's highest one: its ghost slice) */
  int64_t alias_z;                   /* global z of the slice the flag is about: the first occupied slice of the counted
                                        range (own_z0 - 1, the ghost slice, included); -1 without the flag.  Its source is
                                        the highest occupied slice STRICTLY below it that any rank owns.  When alias_z is
                                        the ghost slice only the source's bits are needed (cuberille_recount), no plane */
} cuberille_slab_status;

typedef struct {
  uint64_t n_points;        /* points this call/rank owns */
  uint64_t n_cells;         /* cells this call/rank owns (quads, or 2 triangles per quad) */
  int32_t verts_per_cell;   /* 4 or 3 */
  int32_t reserved;
  /* Device time in milliseconds (HIP events on the context's stream).  ms_total is always measured, ms_pass for volumes of
   * more than 4 Mi voxels (below that ONE event pair brackets the extraction and ms_pass is 0: an event between two kernels
   * costs the stream about 8 us, as much as such a volume's kernels); the five per-stage figures only with
   * cuberille_debug_set_option(ctx, "stage_timing", 1) and are 0 otherwise. */
  float ms_classify;        /* threshold + bit-pack sweep over the volume */
  float ms_count;           /* per-word face / created-corner counts and all prefix sums (one kernel) */
  float ms_scan;            /* 0: the scans run inside the count kernel since ABI 4 (field kept for layout) */
  float ms_emit_points;     /* vertex scatter: AddVertex without the projection (txx:256-276) */
  float ms_project;         /* vertex projection (txx:439-474); with cuberille_set_point_normals on, the normals pass behind it too */
  float ms_emit_cells;      /* quad / triangle scatter incl. the diagonal split (txx:278-332); with cuberille_set_cell_pixels on, the
                               cell-pixel pass behind it too, with cuberille_set_components on the component pass */
  float ms_total;           /* ms_pass + the emit phase (points, projection, cells).  When cuberille_emit_points started the
                               vertex phase ahead of cuberille_emit, the two phases are timed as intervals of their own and
                               added: the device's wait for the host's all-gather in between is in neither.  Inside
                               cuberille_extract_device (no host turn in the middle) it is one interval from the first
                               launch to the last: every further event would idle the stream for about 10 us */
  float ms_pass;            /* classify + count + scan: the pass over the volume.  cuberille_extract_host's chunked upload and
                               cuberille_extract_stream threshold every chunk as it lands, so for those two entries the
                               figure includes the ingestion; after cuberille_recount it is the second count alone */
  uint64_t proj_iterations; /* total iterations of the projection loop */
  /* why the walks ended: the reference's DEBUG_PRINT counters m_ProjectVertexTerminate[0] / [1] (h:336-338; txx:457-459,
   * 470-472, printed at txx:208-214): within the distance threshold / out of steps.  Owned vertices only; a vertex of the
   * ADVANCED branch that stops on its oscillation rule and every vertex of the LINESEARCH branch count in neither. */
  uint64_t proj_stop_threshold;
  uint64_t proj_stop_steps;
  uint64_t n_escaped;       /* THIN_HALO slabs: vertices whose walk left the buffer, waiting for cuberille_reproject_escaped */
} cuberille_result;

typedef struct cuberille_ctx cuberille_ctx;

/* library */
int cuberille_abi_version(void);
/* number of usable gfx950 devices (0 when there is none; never fails) */
int cuberille_device_count(void);
const char *cuberille_last_error(const cuberille_ctx *ctx); /* ctx may be NULL: last create (or cuberille_region_desc) error */

/* context: owns a stream and the device workspace (re-used across calls) */
int cuberille_create(cuberille_ctx **out, int device_id);
void cuberille_destroy(cuberille_ctx *ctx);
/* Optional: takes what the FIRST extraction on a fresh context pays besides its kernels out of that call -- the way the
 * reference's driver times the filter is one cold Update() per process (Testing/CuberilleTest01.cxx:158-160, the filter
 * constructed and its input set before the clock starts).  Loads the code objects and warms the runtime's launch path
 * (one tiny internal extraction, forgotten afterwards) and, `img` non-null, reserves every buffer whose size follows from
 * the image description alone: the device copy of the volume (cuberille_extract_host), the bit volume, the prefix
 * tables, the vertex-word queue, the corner map, the pinned staging ring of a chunked upload.  `prm` may be null (the
 * defaults of txx:33-40).  The drop-in filter calls it from its constructor (no image) and from SetInput (the image's
 * description).  A failed reservation is not an error: the extraction will ask again and report it.  On a context that
 * holds a count, a mesh or an open step the call reserves nothing and runs nothing (growing a buffer moves it, and the
 * count's tables, the bit volume and the mesh stay readable until the next extraction replaces them): that extraction
 * grows the workspace itself. */
int cuberille_warm_up(cuberille_ctx *ctx, const cuberille_image_desc *img, const cuberille_params *prm);
/* run on a caller's hipStream_t instead of the context's own (NULL = back to own) */
int cuberille_set_stream(cuberille_ctx *ctx, void *hip_stream);

/* One call = GenerateData(): upload `host_voxels`, extract, leave the mesh on the device.  Large volumes cross
 * the link in z-chunks through a pinned double buffer filled by a few host threads, and every chunk is thresholded
 * while the next one is in flight, so the call takes about bytes / link rate (pageable caller memory included). */
int cuberille_extract_host(cuberille_ctx *ctx, const cuberille_image_desc *img, const void *host_voxels,
                           const cuberille_params *prm, cuberille_result *res);
/* The same pipeline fed by a PRODUCER instead of a finished host buffer (the reader side of the reference's driver,
 * Testing/CuberilleTest01.cxx:113-117: itk::ImageFileReader inflates a zlib-compressed MetaImage before the filter
 * runs).  `source(user, dst, z0, z1)` writes slices [z0, z1) of the volume, x fastest, (z1 - z0) * Nx * Ny pixels, to
 * `dst` -- pinned staging memory of the library -- and returns 0, or non-zero to give up (CUBERILLE_ERR_SOURCE; the
 * context stays usable).  It is called on the calling thread, for consecutive z ranges in ascending order, every slice
 * exactly once.  While it produces one chunk (inflates the next stretch of the file, say) the previous chunk crosses
 * the link and is thresholded, and the volume never exists as a whole in host memory. */
typedef int (*cuberille_chunk_source)(void *user, void *dst, int64_t z0, int64_t z1);
int cuberille_extract_stream(cuberille_ctx *ctx, const cuberille_image_desc *img, cuberille_chunk_source source, void *user,
                             const cuberille_params *prm, cuberille_result *res);
/* Same with the volume already resident in HBM (`dev_voxels` is a device pointer). */
int cuberille_extract_device(cuberille_ctx *ctx, const cuberille_image_desc *img, const void *dev_voxels,
                             const cuberille_params *prm, const cuberille_slab *slab, cuberille_result *res);

/* The two halves of extract_device, for multi-GPU: count -> (all-gather of counts, prefix on the
 * host) -> emit with this rank's id offsets. */
int cuberille_count(cuberille_ctx *ctx, const cuberille_image_desc *img, const void *dev_voxels,
                    const cuberille_params *prm, const cuberille_slab *slab,
                    uint64_t *n_points, uint64_t *n_cells);
int cuberille_emit(cuberille_ctx *ctx, uint64_t point_id_offset, cuberille_result *res);
/* The same step without a host round trip between count and emit -- the steady state of a multi-GPU driver, and the
 * short way through a small volume.  cuberille_step_begin (arguments of cuberille_count) launches the count AND the part
 * of the emit that needs no id offset back to back and returns without waiting: the launches behind the count are sized
 * from what the previous extraction on this context produced (+25 %), read the real counts from device memory and run
 * only if those fit.  (The first extraction on a context, and configurations without the scratch tables, wait for the
 * counts once instead; the caller sees no difference.)  *dev_row: this rank's row, *row_bytes bytes of device memory
 * that are final when the context's stream gets there.  The caller gathers the rows of all ranks, in rank order, into
 * device memory -- stream-ordered behind this call, e.g. RCCL's all-gather on the same stream; one rank: the row itself
 * -- and calls cuberille_step_end(rows, n_ranks, rank): the cells, with this rank's id offset summed on the device from
 * the rows below it, then the ONE wait of the step.  CUBERILLE_OK: the mesh is in place as after cuberille_emit.
 * CUBERILLE_RETRY: a row carries a flag -- quirk Q1 crossing a slab boundary, counts beyond the sizes guessed, a walk
 * that left a THIN_HALO -- on SOME rank: no rank has written cells (each looks at all rows), the count stands (*res holds
 * n_points / n_cells as cuberille_count would have returned them) and the calls above continue from it on every rank
 * (cuberille_slab_info ... cuberille_emit). */
int cuberille_step_begin(cuberille_ctx *ctx, const cuberille_image_desc *img, const void *dev_voxels,
                         const cuberille_params *prm, const cuberille_slab *slab, const void **dev_row, size_t *row_bytes);
int cuberille_step_end(cuberille_ctx *ctx, const void *dev_rows, int n_ranks, int rank, cuberille_result *res);
/* cuberille_step_begin in two calls, for a driver that sends the neighbour ranks the inside BITS of its boundary slices ahead
 * of their voxels: everything between the sweep and the walk -- faces, vertex ids, prefix sums, the vertex scatter -- reads
 * the 1-bit volume alone (1/32 of the bytes of a float32 slice: microseconds on a link), only the projection walk reads the
 * halo's voxels.  cuberille_step_classify (arguments of cuberille_count; halo_ready_event of the slab is ignored) thresholds
 * the OWNED slices and returns at once; *dev_bits is the bit volume of the buffer, slice z (local) at dev_bits + z *
 * words_per_slice, (Nx+63)/64 words per x-row -- complete for the owned slices when the context's stream gets there.  The
 * driver sends its neighbours the planes of the owned slices they hold as halo and receives, INTO dev_bits, the planes of its
 * own halo slices (every slice of the buffer outside [own_z0, own_z1): they are never thresholded here).
 * cuberille_step_count(halo_bits_event, halo_voxels_event, ...) then continues as cuberille_step_begin does behind its sweep:
 * the count waits for halo_bits_event (recorded by the caller behind the arrival of the planes; null: they are there
 * already), the walk -- alone -- for halo_voxels_event (recorded behind the arrival of the halo's voxels; null likewise).
 * Same row, same cuberille_step_end, same results bit for bit: the planes a neighbour sends are the bits this rank would
 * have computed from the same voxels. */
int cuberille_step_classify(cuberille_ctx *ctx, const cuberille_image_desc *img, const void *dev_voxels,
                            const cuberille_params *prm, const cuberille_slab *slab, uint64_t **dev_bits, size_t *words_per_slice);
int cuberille_step_count(cuberille_ctx *ctx, void *halo_bits_event, void *halo_voxels_event, const void **dev_row, size_t *row_bytes);
/* A rank whose cuberille_step_begin FAILED has no row, yet its peers are on their way into the all-gather of the rows:
 * this writes, into `capacity` bytes of HOST memory, a row that says "this rank failed" (*row_bytes: its size, the same
 * as every row's).  The driver copies it to the device and contributes it to the gather in place of the row it does not
 * have; every peer's cuberille_step_end then returns CUBERILLE_RETRY without writing a cell, and the ranks meet in the
 * driver's synchronous protocol, where the failure is raised on all of them.  Needs no GPU and no context. */
int cuberille_failed_row(void *host_row, size_t capacity, size_t *row_bytes);
/* Optional, between the two: starts the part of the emit that needs no id offset -- head tables, vertex scatter,
 * projection -- and returns at once, so that the GPU works while the caller gathers the other ranks' counts;
 * cuberille_emit then only adds the cells.  A cuberille_recount after it voids what it started. */
int cuberille_emit_points(cuberille_ctx *ctx);
/* Slices a slab buffer must hold below own_z0 and above own_z1 (where the volume does not end) for these
 * parameters: 2 / 1 for the topology, and as far as the projection walk can carry a vertex -- step *
 * sum(relaxation^k, k <= max_steps+1) over the z spacing, from where the walk STARTS: half a voxel under the lattice corner for an
 * axis-aligned image, further under a tilted direction matrix (txx:266-270 take half a spacing off every PHYSICAL axis) -- plus
 * the interpolation cell and the gradient ring.
 * cuberille_count returns CUBERILLE_ERR_HALO for a buffer that holds less.  Needs no GPU. */
int cuberille_required_halo(const cuberille_image_desc *img, const cuberille_params *prm, int64_t *below, int64_t *above);
/* The least a THIN_HALO slab must hold: 2 below / 1 above for the topology (the ghost slice own_z0 - 1 and the slice under
 * it decide the ids on plane own_z0); with the projection on, also the cell a vertex STARTS in and its gradient ring for the
 * vertices on planes own_z0 .. own_z1 -- 2 / 2 for an axis-aligned image (a vertex starts half a voxel under its lattice
 * corner, txx:266-270).  Every slice more is margin a walk may use before it counts as escaped.  Needs no GPU. */
int cuberille_minimum_halo(const cuberille_image_desc *img, const cuberille_params *prm, int64_t *below, int64_t *above);
/* THIN_HALO slabs, after cuberille_emit_points: how many walks left the buffer (waits for the vertex phase; UINT64_MAX:
 * more than the list holds).  When any rank
 * reports some, every rank completes its halo to cuberille_required_halo and the ranks concerned call
 * cuberille_reproject_escaped(buffer, its first global slice, its slice count) -- same pixel type, Nx, Ny and geometry as the
 * counted slab; the counted slab's own buffer is not read again -- which walks exactly those vertices again, from their
 * start; then cuberille_emit as usual.  More escapes than the list holds (2^20): CUBERILLE_ERR_LIMIT, count the slab again
 * with the full halo.  cuberille_emit on a THIN_HALO slab refuses (CUBERILLE_ERR_HALO, the count stands) while walks wait. */
int cuberille_escaped_count(cuberille_ctx *ctx, uint64_t *n_escaped);
int cuberille_reproject_escaped(cuberille_ctx *ctx, const void *dev_voxels, int64_t z_begin, int64_t nz);
/* Vertices created and quads emitted by every OWNED slice of the last count (n_slices = own_z1 - own_z0 entries each; a
 * null array is skipped; waits for the stream).  For a driver that cuts a series of similar volumes into slabs of equal work
 * rather than of equal thickness: the surface of a volume is rarely spread evenly over z. */
int cuberille_slice_counts(cuberille_ctx *ctx, uint64_t *points, uint64_t *quads, size_t n_slices);
/* After cuberille_count on a slab: see cuberille_slab_status. */
int cuberille_slab_info(cuberille_ctx *ctx, cuberille_slab_status *out);

/* Quirk Q1 across a slab boundary (the reference re-uses the vertices of the last occupied slice below a run of
 * empty slices, txx:139-141 before 156-161).  When a slab's first occupied slice has only empty
 * slices below it in the buffer (cuberille_slab_status.alias_source_below_buffer) and a rank below holds an occupied
 * slice zp, four calls reproduce the reference:
 *   below: cuberille_slice_bits_device(zp)        -> the inside bits of slice zp (device pointer, n_words words)
 *   above: cuberille_recount(those bits)          -> the counts with the re-used vertices no longer created
 *   below, after its cuberille_emit:
 *          cuberille_alias_plane_device(zp, ids, points) -> global id and final position of the vertex under every
 *                                                    (x, y) corner key of the plane above slice zp, (nx+1)(ny+1) entries
 *   above: cuberille_set_alias_plane(ids, points); cuberille_emit(...) -> cells that reference those vertices
 * All pointers are device pointers of the calling context's device (the driver moves them between ranks). */
int cuberille_slice_bits_device(cuberille_ctx *ctx, int64_t z_global, const uint64_t **dev_words, size_t *n_words);
int cuberille_recount(cuberille_ctx *ctx, const void *dev_source_bits, uint64_t *n_points, uint64_t *n_cells);
int cuberille_alias_plane_device(cuberille_ctx *ctx, int64_t z_global, uint64_t *dev_ids, float *dev_points);
int cuberille_set_alias_plane(cuberille_ctx *ctx, const uint64_t *dev_ids, const float *dev_points);

/* Result buffers of the last extract/emit (valid until the next call on this context):
 * points = float[3*n_points], cells = uint64[verts_per_cell*n_cells] holding GLOBAL point ids. */
int cuberille_mesh_device(const cuberille_ctx *ctx, const float **d_points, const uint64_t **d_cells);
int cuberille_mesh_download(cuberille_ctx *ctx, float *points, uint64_t *cells);
/* The same mesh in HOST memory the context owns (the reference's driver takes the output right behind Update(),
 * Testing/CuberilleTest01.cxx:161-162): *points = float[3*n_points], *cells = uint64[verts_per_cell*n_cells], valid -- and
 * the caller's to read or write -- until the next count / extraction on the context or cuberille_destroy.  The buffers
 * are kept across extractions (a second mesh of similar size lands in memory that is mapped already: the copy then runs
 * at the link's rate) and are backed by huge pages where the system offers them, first touched by the threads that
 * fill them, so that the first mesh of a process does not wait for a page fault per 4 KiB as a fresh malloc'ed
 * destination of cuberille_mesh_download does.  Repeated calls for the same mesh return the same pointers without
 * copying again.  Either pointer argument may be null. */
int cuberille_mesh_host(cuberille_ctx *ctx, float **points, uint64_t **cells);
/* Gives the host memory behind cuberille_mesh_host back to the system (about 1.125 times the flat mesh, otherwise kept for the
 * context's lifetime: a caller that has copied its mesh out -- the drop-in filter, once its itk::Mesh is filled and
 * SetReleaseHostMeshAfterFill(true) was asked for -- and extracts rarely).  The pointers handed out become invalid; the mesh
 * on the device stays, the next cuberille_mesh_host maps fresh memory.  (ABI 11.) */
int cuberille_release_host_mesh(cuberille_ctx *ctx);

/* Quirk Q3 of the reference, on request.  ComputeGradientImage() (itkCuberilleImageToMeshFilter.txx:478-498) builds the
 * gradient image and its interpolator only while m_GradientInterpolator is null (txx:484) and nothing ever resets it: from
 * the second Update() of a filter object on, whatever the input, the walk of txx:439-474 follows the gradient -- and maps its
 * points through the geometry -- of the image the FIRST projecting Update() saw.  This library evaluates the current
 * volume's gradient by default.  With hold != 0 a context behaves like the reference's filter
 * object: its next extraction with project_vertices on (a whole volume: slabs are refused) also materialises that volume's
 * float gradient image in device memory (12 bytes per voxel) and every later extraction on the context, of any size,
 * geometry or pixel type, walks along it -- results then equal a second Update() of the reference bit for bit (the
 * oracle's cuberille_oracle_run_after).  Offered with CUBERILLE_GRADIENT_CENTRAL and every projection_variant; such
 * extractions take the plain one-lane-per-vertex walk, not the refilling one.  hold == 0 drops the image and returns to the
 * default.  Not to be called between cuberille_step_begin and cuberille_step_end.  (ABI 12.) */
int cuberille_hold_gradient(cuberille_ctx *ctx, int hold);
/* 1 when the context holds a gradient image (dims, if not null, receives its size in voxels; zeros otherwise), else 0. */
int cuberille_gradient_held(cuberille_ctx *ctx, int64_t dims[3]);

/* NEW SYMBOLS (added within ABI 13: no existing struct or symbol changes).
 * The value interpolator of the walk (txx:455): the reference's filter is a template over TInterpolator (h:187-188), and
 * its driver's one alternative is itk::BSplineInterpolateImageFunction<ImageType, float, float> with SetSplineOrder(3)
 * (Testing/CuberilleTest01.cxx:73-74,148-151).  CUBERILLE_INTERP_BSPLINE makes the later extractions on ctx compute
 * that interpolator's coefficient image on the device (ITK's BSplineDecompositionImageFilter, mirror boundaries, the input
 * rounded to the coefficient type first and every axis pass rounded back to it) and evaluate its 64 taps in the default
 * branch of the walk (txx:439-474), the central-difference gradient unchanged.  Accepted: spline_order 3 with
 * (coordinate_bits, coefficient_bits) = (32, 32) or (64, 64) -- <float, float> or <double, double>; anything else is
 * CUBERILLE_ERR_ARGUMENT and leaves the setting as it was.  An extraction with project_vertices on and the B-spline set
 * is refused with CUBERILLE_ERR_ARGUMENT, the context staying usable, on a slab (the prefilter needs whole lines), with a
 * projection_variant other than CUBERILLE_PROJECT_DEFAULT, with CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN, and while the
 * context holds a gradient (cuberille_hold_gradient); everywhere CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN is accepted --
 * extract_host, extract_stream, extract_device and the whole-volume step calls -- so is this.  The coefficient image
 * takes 4 or 8 bytes per voxel of device memory, plus an 8-byte scratch volume for 32-bit coefficients, reserved at the
 * first such extraction and kept.  With stage timing on the prefilter is part of ms_project.  The parity target is
 * itk_lite's restatement of ITK's class (midas-journal-740_amd/itk/itk_lite/itkBSplineLite.h), bit for bit; agreement with
 * ITK's own bytes is unpinned.  CUBERILLE_INTERP_LINEAR restores the default (the other arguments are then ignored): a
 * context that never calls this, or sets LINEAR again, gives the same bytes as before this symbol existed. */
enum { CUBERILLE_INTERP_LINEAR = 0, CUBERILLE_INTERP_BSPLINE = 1 };
int cuberille_set_interpolator(cuberille_ctx *ctx, int kind, int spline_order, int coordinate_bits, int coefficient_bits);
/* NEW SYMBOL (added within ABI 13: no struct changes).  Close the surface at the image border without a padded copy.
 * The reference documents one limitation (h:54-57): no iso-surface pixel may lie on the edge of the image, the caller must pad
 * it by at least one pixel with itk::ConstantPadImageFilter first -- else the mesh has holes wherever the object touches the
 * border.  With pad_width 1, every later whole-volume extraction on ctx of an image I (dims N, start index s, origin, spacing,
 * direction) yields exactly the mesh an extraction with the setting off yields for the image P that filter makes of I: dims
 * N + 2, start index s - 1, the same origin / spacing / direction, P[p] = I[p - 1] inside and pad_value on the one-voxel
 * ring -- the same point ids, order, float bits, cells and walk counters.  The ring is implied, never stored: no copy of the
 * voxels, padded or not, is made on the device (cuberille_extract_device, cuberille_count) or on the host
 * (cuberille_extract_host, cuberille_extract_stream); the 1-bit volume and the rest of the workspace have the padded size
 * (cuberille_warm_up reserves that).  A pad value that is itself >= the iso value is legal and gives what P gives.
 * pad_width: 0 (off, the default: the same bytes as before this symbol existed) or 1; anything else CUBERILLE_ERR_ARGUMENT,
 *   setting unchanged.  (An argument so that a wider border can come without a new symbol.)
 * pad_value / pad_value_int: convert to the pixel type by the rule of iso_value / iso_value_int, checked at the extraction,
 *   where the pixel type is known (out of range or NaN for an integer type: CUBERILLE_ERR_ARGUMENT).  The limits on dims and
 *   index_start then hold for N + 2 and s - 1.
 * Refused with CUBERILLE_ERR_ARGUMENT and a message, the context left usable -- each of these would need the ring in a second
 * image or across ranks, and is deliberately not part of this setting: always, a slab that is not the whole volume, the
 * cuberille_step_* calls and cuberille_group_extract_host with a member that has it set; with project_vertices on, the
 * B-spline interpolator, a held gradient (cuberille_hold_gradient), CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN and the ADVANCED and
 * LINESEARCH projection branches.
 * While the setting is on, cuberille_debug_bits speaks the padded frame (rows of N0 + 2 voxels, N1 + 2 rows, N2 + 2 slices);
 * so does cuberille_slice_occupancy (N2 + 2 slices, the ring's first); so does cuberille_slice_counts (N2 + 2 entries). */
int cuberille_set_border(cuberille_ctx *ctx, int pad_width, double pad_value, int64_t pad_value_int);
/* NEW SYMBOLS (added within ABI 13: no struct changes).  Extract a box of a larger volume in place, without a cropped copy.
 * With a region set, `img` still describes the whole buffer the caller hands over -- its dims, its index_start s, origin,
 * spacing and direction -- and every later whole-volume extraction on ctx yields exactly the mesh an extraction with the
 * setting off yields for the image C that itk::ExtractImageFilter / RegionOfInterestImageFilter (the index kept) makes of it:
 * dims `size`, start index s + start, the same origin / spacing / direction, C[p] = I[p + start] -- the same point ids, order,
 * float bits, cells and walk counters.  `start` is a position in the buffer (x, y, z).  Voxels outside the box never enter a
 * result: every clamp (ZeroFluxNeumann, the interpolators' Start/EndIndex) happens at the box's faces, as it would on the copy.
 * No copy of the voxels, cropped or not, is made on the device (cuberille_extract_device, cuberille_count + cuberille_emit):
 * the 1-bit volume and the rest of the workspace have the box's size, a pitched threshold sweep and a walk that knows the
 * buffer's row and slice pitch read the caller's buffer.  cuberille_extract_host uploads the box alone, straight from the
 * caller's image (one strided copy below a GiB, from there the chunk pipeline, its staging threads gathering the box's rows);
 * no host-side crop is allocated.  cuberille_warm_up reserves for `size`, not for dims.
 * cuberille_set_region: size all zero, or both pointers null, turns the region off (the default: the same bytes as before the
 *   symbol existed); a box equal to the whole buffer is legal and gives the same bytes as off.  CUBERILLE_ERR_ARGUMENT, the
 *   setting unchanged, for a negative start or a non-positive size.  The box is checked against the buffer at the extraction,
 *   where dims is known, by cuberille_region_desc.
 * cuberille_region_desc (needs no GPU, no context): writes C's description; the single validator.  CUBERILLE_ERR_ARGUMENT for
 *   a negative start, a non-positive size or a box that leaves the buffer; CUBERILLE_ERR_LIMIT when s + start leaves +-2^30 or
 *   s + start + size exceeds 2^31 - 1 (the kernels add a start index and a position in `int`).  Region off: *cropped = *img.
 *   The text of a refusal: cuberille_last_error(NULL), kept per thread like that of a failed cuberille_create.
 * Refused with CUBERILLE_ERR_ARGUMENT and a message, the context left usable, each deliberately not part of this setting: a slab
 * that is not the whole volume; the cuberille_step_* calls; cuberille_extract_stream; cuberille_group_extract_host with a
 * member that has a region; cuberille_set_border together with a region; with project_vertices on, the B-spline interpolator,
 * a held gradient (cuberille_hold_gradient), CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN and the ADVANCED and LINESEARCH branches.
 * Region + border is the obvious follow-up and NOT part of this: a box that cuts through the object leaves the surface open at
 * the box's faces, exactly as the reference leaves it open at the faces of the cropped copy.
 * While the setting is on, cuberille_debug_bits, cuberille_slice_occupancy and cuberille_slice_counts speak the box's frame
 * (rows of size[0] voxels, size[1] rows, size[2] slices). */
int cuberille_set_region(cuberille_ctx *ctx, const int64_t start[3], const int64_t size[3]);
int cuberille_region_desc(const cuberille_image_desc *img, const int64_t start[3], const int64_t size[3],
                          cuberille_image_desc *cropped);
/* Mesh a label or a value band in place (new symbols within ABI 13, no struct changed).  With a band set, every later
 * whole-volume extraction of an image I of pixel type T gives exactly the mesh the same context with the band off gives for
 *   B(u) = (lower <= I(u) && I(u) <= upper) ? inside : outside        -- all four values are T; a NaN pixel is outside --
 * the image itk::BinaryThresholdImageFilter<Image<T>, Image<T>> makes of I: the same dims, start index, origin, spacing and
 * direction; the iso value and every other parameter stay the caller's and apply to B.  The same counts, ids, order and cells,
 * and with project_vertices on the same coordinate bytes: the walk interpolates B, not I.  B is never stored and nothing the
 * size of the voxels is allocated: the sweep evaluates the band in place of the threshold (!(B < iso) takes two values, so the
 * bit is "in the band" XOR !(outside < iso); where !(inside < iso) says the same the bit volume is constant and the mesh empty),
 * the walk turns every pixel it loads into inside or outside, in T, before any arithmetic.
 * v = {lower, upper, inside, outside}; the 64-bit integer pixel types take vi (the same 64 bits for a uint64 past 2^63), like
 * the iso value; the floating types convert v like the iso value (a C cast).
 * cuberille_set_band: on = 0 restores the default (the same bytes as before the symbol existed; v and vi may be null).  A NaN
 *   bound is refused at once; the rest is checked at the extraction, where the pixel type is known, by cuberille_band_check.
 * cuberille_band_check (needs no GPU, no context): the single validator.  CUBERILLE_ERR_ARGUMENT for a value the pixel type
 *   does not hold -- outside its range, or a fraction for an integer type: a bound cut off like a C cast would move the band
 *   by a label --, for lower > upper (ITK throws there) and for a NaN bound.  The text of a refusal:
 *   cuberille_last_error(NULL), kept per thread like that of a failed cuberille_create.
 * Offered: cuberille_extract_device, cuberille_extract_host (the chunked upload included) and cuberille_count +
 * cuberille_emit on a whole volume, project_vertices off and on, quads and triangles, every pixel type.
 * Refused with CUBERILLE_ERR_ARGUMENT and a message that names the band, the context left usable, each because it would need
 * B in a second image or across ranks: a slab that is not the whole volume; the cuberille_step_* calls;
 * cuberille_group_extract_host with a member that has a band; cuberille_extract_stream; cuberille_set_border or
 * cuberille_set_region together with a band; with project_vertices on, the B-spline interpolator, a held gradient
 * (cuberille_hold_gradient), CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN and the ADVANCED and LINESEARCH branches. */
int cuberille_set_band(cuberille_ctx *ctx, int on, const double v[4], const int64_t vi[4]);
int cuberille_band_check(int pixel_type, const double v[4], const int64_t vi[4]);
/* Point normals (new symbols within ABI 13, no struct changed).  A cuberille mesh is made of axis-aligned quads: its face
 * normals are six constant directions.  What shades the projected surface smoothly is the gradient of the image at each vertex --
 * the vector the walk evaluates in every pass and throws away (normal = m_GradientInterpolator->Evaluate(vertex);
 * normal.Normalize(), txx:451-452).  With the setting on, every later extraction also leaves N(p) for every point p, one
 * definition for every route and pixel type: the three floats of p exactly as they stand in the points buffer -- behind the walk,
 * or at the lattice start with project_vertices off -- go through the steps of the walk's contract: I4 the
 * point to a continuous index in double; I5 the eight sites clamped to the image; I6 at each site the central-difference gradient
 * in float with the direction transform; I7 their linear interpolation (the sum in double in counter order 0..7, zero weights
 * skipped, stopped once the weights sum to exactly 1, each component narrowed to float); I8 Normalize(): the double sqrt of the
 * sum of squares, each component float(double(c) / norm).  Quirk Q4: there is no zero guard -- a zero gradient (a plateau)
 * gives NaN normals and they stay NaN.  N points the way the reference's `normal` points: TOWARDS INCREASING PIXEL VALUES, which
 * for an object brighter than its surroundings is INTO the object; it is not flipped.  The gradient is the central one of the
 * voxels with the B-spline interpolator too.  With a source view the image is the view's frame: the padded image
 * (cuberille_set_border), the box (cuberille_set_region), B (cuberille_set_band).
 * The normals are written by a pass of their own behind the walk (behind the vertex scatter with the projection off), one visit
 * per vertex; with stage timing on its time is part of ms_project.  The buffer is one more row of the workspace, 12 bytes per
 * point, sized where the points are (cuberille_warm_up runs its internal extraction with the setting as it stands: on, the
 * pass's code is loaded and the row exists; off, nothing is reserved for it).  Points, cells and counters are the bytes of the
 * same extraction with the setting off.
 * cuberille_set_point_normals: on != 0 / 0 (the default: nothing allocated, nothing launched, every result as before the symbol
 *   existed; turning it off also frees the row and the normals of the last mesh).  Not between cuberille_step_begin and _end.
 * cuberille_normals_device: *d_normals = float[3*n_points] of the last extraction in point-id order, in the library's buffer
 *   (valid until the next call on the context; it may be null for an empty mesh).  cuberille_normals_download: the same into host memory.
 *   Both: CUBERILLE_ERR_STATE with a message when the last extraction ran with the setting off (or there is no mesh).  The point-id
 *   offset of cuberille_emit does not touch them: entry i belongs to the i-th point of the buffer.
 * cuberille_mesh_write_vtk on a context that holds normals appends "POINT_DATA n" / "NORMALS normals float" and the vectors, in the
 *   points' number format; with the setting off the file is byte for byte what it always was.
 * Offered: cuberille_extract_host, cuberille_extract_device, cuberille_extract_stream, cuberille_count + cuberille_emit_points /
 * cuberille_emit on a whole volume; project_vertices on or off, every projection branch, both interpolators, each source view
 * where that view is offered.  Refused with CUBERILLE_ERR_ARGUMENT and a message that says "point normals", the context left
 * usable: a slab that is not the whole volume; the cuberille_step_* calls; cuberille_group_extract_host with a member that has the
 * setting on; a context holding a gradient (cuberille_hold_gradient: the reference would evaluate the stale image there, and which
 * image is meant is ambiguous); CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN. */
int cuberille_set_point_normals(cuberille_ctx *ctx, int on);
int cuberille_normals_device(cuberille_ctx *ctx, const float **d_normals);
int cuberille_normals_download(cuberille_ctx *ctx, float *normals);
/* Test aid (new symbol): the bytes of device memory the context's workspace holds at this moment -- the capacities of all its
 * buffers added up (what cuberille_warm_up and the extractions reserved and kept). */
int cuberille_debug_device_bytes(cuberille_ctx *ctx, size_t *bytes);
/* Cell pixels (new symbols within ABI 13, no struct changed).  Which voxel a face belongs to: behind every cell it adds the
 * reference keeps a commented-out mesh->SetCellData( id, (OutputPixelType)0 ) (txx:314, 321, 330), and the maintained successor of
 * the filter offers the pixel there as a switch.  With the setting on, every later extraction also leaves one value per cell, one
 * definition for every route, pixel type and source view: quad (u, f) -- it exists when u is inside and its neighbour across face f
 * is not; quads are in voxel raster order, then f ascending -- carries I(u), the pixel of its INSIDE voxel u in the image's own
 * pixel type, copied byte for byte (a NaN keeps its payload, -0.0 stays -0.0, an 8-byte integer no double holds stays exact).  With
 * generate_triangles cells 2k and 2k + 1 both carry the pixel of quad k.  It does not depend on the projection, its branch, the
 * interpolator or the gradient.  With a source view I is the view's frame BEFORE any band mapping: the padded image
 * (cuberille_set_border; a quad whose inside voxel lies on the ring -- possible when the constant is not below the iso value --
 * carries the constant), the box (cuberille_set_region), and with cuberille_set_band the caller's RAW pixel, not `inside` /
 * `outside`.  That is deliberate: the mesh is that of the thresholded image B, but B's cell data would be one constant and say
 * nothing, while the raw pixel says which label -- one extraction of the band [1, 255] gives the outer surface of all labels, to be
 * split per label afterwards.
 * The values are written by a pass of its own behind the cell pass, one lane per quad and one load each; with stage timing on its
 * time is part of ms_emit_cells.  The buffer is one more row of the workspace, one pixel per cell, sized where the cells are
 * (cuberille_warm_up runs its internal extraction with the setting as it stands: on, the pass's code is loaded and the row exists;
 * off, nothing is reserved for it).  Points, cells and counters are the bytes of the same extraction with the setting off.
 * With the setting on cuberille_emit READS THE VOXELS: a caller of cuberille_count + cuberille_emit keeps the voxel buffer it
 * counted valid and unchanged until cuberille_emit returns.
 * cuberille_set_cell_pixels: on != 0 / 0 (the default: nothing allocated, nothing launched, every result as before the symbol
 *   existed; turning it off also frees the row and the cell pixels of the last mesh).  Not between cuberille_step_begin and _end.
 * cuberille_cell_pixels_device: *d_pixels = n_cells values of the last extraction in cell order, in the library's buffer (valid
 *   until the next call on the context; null for an empty mesh), *pixel_type (may be null) their CUBERILLE_PIX_* type.
 * cuberille_cell_pixels_download: the same into host memory; CUBERILLE_ERR_ARGUMENT when capacity_bytes is below n_cells pixels.
 *   Both: CUBERILLE_ERR_STATE with a message when the last extraction ran with the setting off (or there is no mesh).  The
 *   point-id offset of cuberille_emit does not touch them.
 * cuberille_mesh_write_vtk on a context that holds cell pixels appends, behind the polygons and behind the POINT_DATA / NORMALS
 *   block where there is one, "CELL_DATA n" / "SCALARS pixel <vtk type> 1" / "LOOKUP_TABLE default" and one value per line
 *   (integers in decimal, float32 as %.9g, float64 as %.17g; the 8-byte integers as vtktypeint64 / vtktypeuint64); with the
 *   setting off the file is byte for byte what it was.
 * Offered: cuberille_extract_host (chunked upload included), cuberille_extract_device, cuberille_extract_stream, cuberille_count +
 * cuberille_emit_points / cuberille_emit on a whole volume; quads and triangles, the projection on or off, every branch, both
 * interpolators, a held or recursive-Gaussian gradient, each source view where that view is offered.  Refused with
 * CUBERILLE_ERR_ARGUMENT and a message that says "cell pixels", the context left usable: a slab that is not the whole volume; the
 * cuberille_step_* calls; cuberille_group_extract_host with a member that has the setting on. */
int cuberille_set_cell_pixels(cuberille_ctx *ctx, int on);
int cuberille_cell_pixels_device(cuberille_ctx *ctx, const void **d_pixels, int *pixel_type);
int cuberille_cell_pixels_download(cuberille_ctx *ctx, void *out, size_t capacity_bytes);
/* Surface components (new symbols within ABI 13, no struct changed).  What a caller of itk::ConnectedRegionsMeshFilter does with the
 * mesh -- find the connected surfaces, count them, keep the largest, drop the specks -- on the device, where the mesh already is.
 * One definition for every route, pixel type and source view, quads or triangles, on the final mesh exactly as
 * cuberille_mesh_device hands it out (n_points points, n_cells cells): two points are JOINED when one cell holds both; a COMPONENT
 * is a class of the transitive closure; a point that no cell holds is a component of its own with zero cells; components are
 * numbered 0 .. K-1 in the order of their smallest point index.  The point index is the position in `points`: with
 * cuberille_emit(offset) the cells hold index + offset, the pass takes the offset off and the labels never carry it.  A lattice
 * corner is one vertex, so voxels that touch at an edge or a corner only are one component.  The result is a pure function of the
 * mesh; with generate_triangles the point labels and K are those of the quads and the counts exactly doubled.
 *   point_component  uint32[n_points]  the number of the point's component
 *   cell_component   uint32[n_cells]   the component of the cell's first point, in cell order
 *   component_cells  uint64[K]         the cells per component
 * A lock-free union-find over the cells, a scan that numbers the roots and a relabelling pass run behind the cell pass (and behind
 * the cell-pixel pass where that is on); with stage timing on their time is part of ms_emit_cells.  The rows are buffers of their
 * own, sized where the points and cells are: 16 B per point, 4 B per cell and the scan's block sums.  Points, cells and counters
 * are the bytes of the same extraction with the setting off.  Labels are 32-bit: an extraction of 2^32 points or more is refused.
 * cuberille_set_components: on != 0 / 0 (the default: nothing allocated, nothing launched, every result as before the symbol
 *   existed; turning it off also frees the rows and the components of the last mesh).  Not between cuberille_step_begin and _end.
 * cuberille_components_info: *n_components = K of the last extraction.
 * cuberille_components_device: the three rows of the last extraction in the library's buffers (valid until the next call on the
 *   context); each pointer may be null if not wanted; null results for an empty mesh.
 * cuberille_components_download: the same into host memory, each pointer null if not wanted; CUBERILLE_ERR_ARGUMENT when
 *   component_cells is wanted and capacity_components is below K.
 *   All three: CUBERILLE_ERR_STATE with a message when the last extraction ran with the setting off (or there is no mesh).
 * cuberille_mesh_write_vtk on a context that holds components writes "SCALARS component unsigned_int 1" / "LOOKUP_TABLE default"
 *   twice: in POINT_DATA (behind NORMALS where there are any) the point labels, in CELL_DATA (behind the cell pixels' array where
 *   there is one) the cell labels, creating either block where it does not yet exist; with the setting off the file is byte for
 *   byte what it was.
 * Offered: cuberille_extract_host, cuberille_extract_device, cuberille_extract_stream, cuberille_count + cuberille_emit_points /
 * cuberille_emit on a whole volume; with every source view, and with point normals and cell pixels on as well (it reads the mesh,
 * not the voxels).  Refused with CUBERILLE_ERR_ARGUMENT and a message that says "components", the context left usable: a slab that
 * is not the whole volume; the cuberille_step_* calls; cuberille_group_extract_host with a member that has the setting on -- a
 * component does not stop at a slab's face. */
int cuberille_set_components(cuberille_ctx *ctx, int on);
int cuberille_components_info(cuberille_ctx *ctx, uint64_t *n_components);
int cuberille_components_device(cuberille_ctx *ctx, const uint32_t **d_point_component, const uint32_t **d_cell_component,
                                const uint64_t **d_component_cells);
int cuberille_components_download(cuberille_ctx *ctx, uint32_t *point_component, uint32_t *cell_component,
                                  uint64_t *component_cells, size_t capacity_components);
/* Point scalars (new symbols within ABI 13, no struct changed).  The value of ANOTHER image on the surface: what a host loop of
 * interpolator->SetInputImage(other); interpolator->Evaluate(point) over mesh->GetPoints() gives -- the intensity volume under a
 * surface of its label volume, a PET or a dose grid under a surface of the CT, the next time step -- without the mesh leaving the
 * device.  With the extraction's own image as the second one it is the interpolated value at each final vertex, whose distance from
 * the iso value is what the walk stopped on.
 * Image B, the second image: any of the ten pixel types under a description of its own (dims, spacing, origin, direction,
 * index_start), whole and contiguous, x fastest.  One definition for every route, pixel type and source view of the extraction:
 * for each point p of the final mesh the three floats as the points buffer holds them (behind the walk, or the lattice start with
 * project_vertices off; behind cuberille_keep_components on the kept mesh), widened to double,
 *   1. cv = p - origin_B; ci[r] = ((0 + m[r][0]*cv[0]) + m[r][1]*cv[1]) + m[r][2]*cv[2] with m B's point-to-index matrix, built
 *      without contraction (ci = cv where m is the unit matrix): ci is in B's INDEX space;
 *   2. p is inside B when index_start_k - 0.5 <= ci_k && ci_k < index_start_k + n_k - 0.5 on every axis; a NaN coordinate
 *      (quirk Q4) fails the comparison and is outside;
 *   3. inside, the value is itk::LinearInterpolateImageFunction<B, double>::Evaluate(p) under the contract of DESIGN.md section 3:
 *      the cell from floor(ci), the eight neighbours clamped into B's buffered region (I5), each pixel converted by (double) -- a
 *      64-bit integer past 2^53 rounds --, the sum in double in counter order, zero weights skipped, stopped once the weights sum
 *      to exactly 1 (I7);
 *   4. outside, outside_value with its 64 bits as given: a NaN's payload and -0.0 survive.
 * The output is one double per point in point order.  A pass of its own behind the walk (and behind the normals' pass) writes
 * it, one lane per vertex; with stage timing on its time is part of ms_project.  Points, cells, normals, cell pixels, components
 * and counters are the bytes of the same extraction with the setting off.
 * cuberille_set_point_scalars: img == NULL turns the setting off (the default: nothing allocated, nothing launched, every result
 *   as before the symbols existed; it frees the row, its spare and the library's copy of B).  CUBERILLE_MEM_HOST: the library
 *   uploads a copy of its own at the call and waits for it, the caller's memory is free on return; the copy lives until the
 *   setting goes off, is replaced, or the context is destroyed, and counts in cuberille_debug_device_bytes.  CUBERILLE_MEM_DEVICE:
 *   (The upload is ONE plain copy on the context's stream whatever the size -- the chunk pipeline that cuberille_extract_host
 *   takes for a GiB and more is not used here: a caller with an image that large uploads it as it sees fit and hands it over
 *   with CUBERILLE_MEM_DEVICE.  The new copy is complete before an earlier one is freed -- for a moment the context holds
 *   both -- and a call that fails, for lack of memory say, leaves the setting exactly as it was, off or on with the earlier
 *   image.)
 *   the pointer is borrowed -- valid and filled until the setting goes off, read on the context's stream; it may be the very
 *   buffer being extracted.  Not between cuberille_step_begin and _end.
 * cuberille_point_scalars_device: *d_scalars = double[n_points] of the last extraction in the library's buffer (valid until the
 *   next call on the context; null for an empty mesh).  cuberille_point_scalars_download: the same into host memory;
 *   CUBERILLE_ERR_ARGUMENT when capacity_bytes is below 8 * n_points.  Both: CUBERILLE_ERR_STATE with a message when the last
 *   extraction ran with the setting off (or there is no mesh).
 * cuberille_keep_components compacts the row with the others: point_scalars' = point_scalars[kp].
 * cuberille_mesh_write_vtk on a context that holds point scalars writes "SCALARS point_scalar double 1" / "LOOKUP_TABLE default"
 *   last in POINT_DATA (opening the block where none exists), one %.17g per line; with the setting off the file is byte for byte
 *   what it was.
 * Offered: cuberille_extract_host, cuberille_extract_device, cuberille_extract_stream, cuberille_count + cuberille_emit_points /
 * cuberille_emit on a whole volume; every source view, both interpolators, every projection and gradient variant, a held gradient
 * (it reads the points, not the first image).  Refused with CUBERILLE_ERR_ARGUMENT and a message that says "point scalars", the
 * context left usable: a slab that is not the whole volume; the cuberille_step_* calls; cuberille_group_extract_host with a member
 * that has the setting on; a description the library would refuse as an input image; a null `voxels`; an unknown `location`.
 * Out of scope: nearest-neighbour and B-spline sampling of B; vector images or several second images; slabs, steps and groups; a
 * count of the outside points (it is isnan or == outside_value on the row). */
enum { CUBERILLE_MEM_HOST = 0, CUBERILLE_MEM_DEVICE = 1 };
int cuberille_set_point_scalars(cuberille_ctx *ctx, const cuberille_image_desc *img, const void *voxels, int location,
                                double outside_value);           /* img == NULL: off */
int cuberille_point_scalars_device(cuberille_ctx *ctx, const double **d_scalars);
int cuberille_point_scalars_download(cuberille_ctx *ctx, double *out, size_t capacity_bytes);
/* Keep the largest surface, or drop the specks (new symbols within ABI 13, no struct changed): the last mesh of ctx -- one that
 * came with components -- is replaced on the device by the part of it that lies in the kept components, order preserved.
 *   CUBERILLE_KEEP_LARGEST    the one component with the most cells; a tie goes to the smaller component number; K = 0 keeps
 *                             nothing.  n, host_mask and mask_len are ignored.
 *   CUBERILLE_KEEP_MIN_CELLS  every component with component_cells[k] >= n (cells as component_cells counts them: with
 *                             generate_triangles a quad is two).  n = 0 keeps everything, components of zero cells included.
 *   CUBERILLE_KEEP_MASK       component k is kept when host_mask[k] != 0: host memory of exactly K bytes (mask_len != K, or a null
 *                             mask with K > 0: CUBERILLE_ERR_ARGUMENT).  The "specified regions" case; a top-n selection is the
 *                             caller's, from component_cells (K values).
 * With keepK[k] the decision, kp = keepK[point_component], kc = keepK[cell_component], new_index = cumsum(kp) - 1 and
 * new_number = cumsum(keepK) - 1:
 *   points' = points[kp], normals' = normals[kp]; cells' = new_index[cells[kc] - offset] + offset (the offset of cuberille_emit
 *   stays in the ids); cell pixels' = cell pixels[kc], bit for bit; point_component' = new_number[point_component[kp]],
 *   cell_component' = new_number[cell_component[kc]]; component_cells' = component_cells[keepK]; K' = the kept.
 * Every point of a kept component is kept and the compaction is stable, so the new rows are exactly the components of the new
 * mesh, numbered by smallest point index: a second call on the result is legal and composes, LARGEST behind LARGEST changes
 * nothing.  Afterwards cuberille_mesh_device / _download / _host / _write_vtk, cuberille_normals_*, cuberille_cell_pixels_* and
 * cuberille_components_* speak of the kept mesh (pointers handed out before the call are void).  *n_points, *n_cells and
 * *n_components receive the new sizes, *ms the device time of the call from one event pair; each pointer may be null.  The walk
 * counters and the ms_* fields of the extraction's cuberille_result, cuberille_slice_counts, cuberille_debug_bits and the sizes
 * that steer the next blind launch stay the extraction's; the next extraction on the context gives what a fresh context gives.
 * On the device: the decision per component, three exclusive scans (components, points, cells) whose totals reach the host in
 * one read, and a scatter out of place into spare rows sized by the kept counts -- buffers of the context, reserved by this call
 * alone and freed by cuberille_set_components(ctx, 0) -- after which the buffers change places.  When everything is kept no byte
 * moves; when nothing is kept the mesh is empty (null component pointers, empty downloads, K = 0).
 * Refused, the context left usable and the mesh as it was: CUBERILLE_ERR_STATE with a message that says "components" when
 * there is no mesh, the last extraction ran with components off, the mesh is a slab's, or a step is open; CUBERILLE_ERR_ARGUMENT
 * for an unknown rule or the mask errors above; CUBERILLE_ERR_LIMIT with 2^32 cells or more (the cell positions are 32-bit
 * sums); CUBERILLE_ERR_HIP when a row cannot be reserved -- every row is reserved before the first scatter. */
enum { CUBERILLE_KEEP_LARGEST = 0, CUBERILLE_KEEP_MIN_CELLS = 1, CUBERILLE_KEEP_MASK = 2 };
int cuberille_keep_components(cuberille_ctx *ctx, int rule, uint64_t n, const uint8_t *host_mask, size_t mask_len,
                              uint64_t *n_points, uint64_t *n_cells, uint64_t *n_components, float *ms);
/* Test aid (new symbol): the coefficient image of the last B-spline extraction on ctx (one that projected at least one
 * vertex), x fastest, coefficient_bits wide.  CUBERILLE_ERR_STATE when there is none, CUBERILLE_ERR_ARGUMENT when
 * capacity_bytes is smaller than the image. */
int cuberille_bspline_coefficients(cuberille_ctx *ctx, void *host_out, size_t capacity_bytes);
/* Test aid (new symbol): 1 when ctx holds the coefficient image of a B-spline extraction -- dims receives its size in voxels
 * (x, y, z) and coefficient_bits its width (32 or 64) -- else 0 (zeros written).  Either pointer may be null. */
int cuberille_bspline_coefficients_info(cuberille_ctx *ctx, int64_t dims[3], int *coefficient_bits);

/* NEW SYMBOLS (added within ABI 13: no existing struct or symbol changes).
 * A context group: N contexts driven together by one call, for a caller that holds the whole volume in host memory (the
 * reference's driver: SetInput(image); Update()) on a node with several GPUs.  Member i owns slab i of the volume, slabs of
 * equal thickness along z; its buffer is the owned range widened by cuberille_required_halo (the full halo, never
 * CUBERILLE_SLAB_THIN_HALO) and clipped to the volume, uploaded straight from the caller's image on the member's own stream
 * and link -- no member needs another's voxels, so there is no halo exchange, no collective and no peer-to-peer copy.  The
 * counts are summed on the host, quirk Q1 across a cut (the four calls above) is handed over through host memory, and the
 * slabs' meshes land in disjoint ranges of one host mesh the group owns: the same ids, cell order and bits as
 * cuberille_extract_host of the whole volume on one context.  Device ids may repeat (N contexts on one GPU share its link:
 * that measures the group's overhead, not scaling).  Not thread-safe; distinct groups are independent.
 * cuberille_group_create: 1 <= n <= 64, else CUBERILLE_ERR_ARGUMENT (the text of a failed create: cuberille_group_last_error(NULL)).
 * cuberille_group_context: member i, e.g. for cuberille_debug_set_option; null outside [0, n).  Do not extract on it directly
 *   between a group extraction and the reads of its mesh.
 * cuberille_group_plan (needs no GPU): the cuts the group would use for this image and these parameters.  *n_used = min(n, Nz)
 *   members take part; bounds[4 i .. 4 i + 3] = own_z0, own_z1, buf_z0, buf_z1 of slab i (room for 4 n entries).  Slab i's
 *   description is the image's with dims[2] = buf_z1 - buf_z0, its cuberille_slab {Nz, buf_z0, own_z0, own_z1, 0, 0}.
 *   CUBERILLE_ERR_ARGUMENT for n outside 1 .. 64 and for CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN with projection (it needs
 *   whole lines, as on any slab).
 * cuberille_group_warm_up: cuberille_warm_up of every member with its slab's description (img may be null).
 * cuberille_group_extract_host: one host thread per slab uploads and counts its slab (below a GiB per slab one plain copy,
 *   from a GiB the chunked pipeline of cuberille_extract_host; the host staging threads of ONE context are split between the
 *   slabs, at least one each) and starts its vertex phase when no other slab can change its counts; the host then plans and
 *   stages quirk Q1's hand-overs, the slabs emit (those of a hand-over in rank order, the others at once).  *res: n_points,
 *   n_cells and the walk counters summed over the slabs, verts_per_cell as usual, every ms_* field the LARGEST of the slabs'
 *   (they run side by side).  Refused with CUBERILLE_ERR_ARGUMENT and a message: the recursive-Gaussian gradient with
 *   projection, a member with the B-spline interpolator set (cuberille_set_interpolator), a member holding a gradient
 *   (cuberille_hold_gradient).  A failure on any slab drains every member's streams and returns its status; the text names
 *   the slab and the call.  The group stays usable.
 * cuberille_group_slab_result: slab i's own result of the last extraction (i < n_used).
 * cuberille_group_mesh_host / _release_host_mesh / _mesh_write_vtk: as cuberille_mesh_host / cuberille_release_host_mesh /
 *   cuberille_mesh_write_vtk, for the assembled mesh (cells hold global ids).
 * cuberille_group_debug_fail_alloc: failure drill -- the n-th device allocation that slab `slab`'s thread makes during the
 *   upload and count of the NEXT extraction reports out-of-memory (slab -1: every slab's; n < 0: off). */
typedef struct cuberille_group cuberille_group;
int cuberille_group_create(cuberille_group **out, const int *device_ids, int n);
void cuberille_group_destroy(cuberille_group *g);
const char *cuberille_group_last_error(const cuberille_group *g);
cuberille_ctx *cuberille_group_context(cuberille_group *g, int i);
int cuberille_group_plan(const cuberille_image_desc *img, const cuberille_params *prm, int n, int64_t *bounds, int *n_used);
int cuberille_group_warm_up(cuberille_group *g, const cuberille_image_desc *img, const cuberille_params *prm);
int cuberille_group_extract_host(cuberille_group *g, const cuberille_image_desc *img, const void *host_voxels,
                                 const cuberille_params *prm, cuberille_result *res);
int cuberille_group_slab_result(const cuberille_group *g, int i, cuberille_result *res);
int cuberille_group_mesh_host(cuberille_group *g, float **points, uint64_t **cells);
int cuberille_group_release_host_mesh(cuberille_group *g);
int cuberille_group_mesh_write_vtk(cuberille_group *g, const char *path, int n_threads);
int cuberille_group_debug_fail_alloc(cuberille_group *g, int slab, int64_t n);

/* Flat-mesh file output (replaces the itk::Mesh fill + itk::VTKPolyDataWriter pass of
 * Testing/CuberilleTest01.cxx:161-187 for callers that keep the flat buffers): legacy-ASCII VTK POLYDATA in
 * the layout of that writer (header lines, "POINTS n float", "POLYGONS m k"), coordinates with 9 significant
 * digits.  Checked byte for byte against the itk_lite writer shipped in this repository; ITK's own writer was
 * never run here, so equality with ITK's bytes (its number formatting) is unpinned.  Formatted by `n_threads` host threads
 * (0 = one per core, at most 32).  The first form writes host buffers and needs no GPU (multi-GPU: rank 0
 * passes the rank-ordered concatenation, whose ids are already global); the second downloads the context's
 * last mesh first and refuses a slab mesh (its cells reference points of the rank below). */
int cuberille_write_vtk_buffers(const char *path, const float *points, uint64_t n_points,
                                const uint64_t *cells, uint64_t n_cells, int verts_per_cell, int n_threads);
int cuberille_mesh_write_vtk(cuberille_ctx *ctx, const char *path, int n_threads);

/* Introspection used by the parity tests: copy the packed inside-bit volume of the last
 * count ((Nx+63)/64 uint64 words per x-row, rows in (z,y) raster order) to `words`. */
int cuberille_debug_bits(cuberille_ctx *ctx, uint64_t *words, size_t n_words);
/* Per buffer slice: non-zero when the slice holds at least one inside voxel.  The multi-GPU
 * driver gathers these to detect the empty-slice aliasing quirk (Q1) crossing a slab boundary. */
int cuberille_slice_occupancy(cuberille_ctx *ctx, uint32_t *occupied, size_t n_slices);
/* Development switches of one context (kernel variants, dropping a scratch table to exercise the fallback
 * path): name = a field of cuberille::Tuning (csrc/cuberille_internal.h), or "defaults" to reset them all.
 * Results never depend on them, only speed and memory.  Used by the parity tests and the ablation scripts.
 * One more name, "fail_alloc_at" = n, is a failure drill: the n-th device allocation the CALLING THREAD makes from
 * now on (through any context) reports out-of-memory (-1 or "defaults": off).  A required buffer then gives
 * CUBERILLE_ERR_HIP and leaves the context usable; an optional scratch table is done without. */
int cuberille_debug_set_option(cuberille_ctx *ctx, const char *name, int64_t value);
/* Measurement aid for the PCIe-inclusive numbers: seconds this context's device takes to receive `bytes` from
 * pinned host memory (64 MiB copies back to back on one stream) -- the link rate cuberille_extract_host is held to. */
int cuberille_debug_h2d_seconds(cuberille_ctx *ctx, size_t bytes, double *seconds);

#ifdef __cplusplus
}
#endif
#endif
