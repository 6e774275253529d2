// Flat-buffer VTK writer (host code).
//
// Replaces, for callers that hold the flat mesh buffers, the itk::Mesh fill + itk::VTKPolyDataWriter pass of
// Testing/CuberilleTest01.cxx:161-187: same legacy-ASCII POLYDATA bytes as the writer the unchanged driver
// uses (9 significant digits, "x y z" per point, "k id0 .. idk-1" per polygon), formatted by a pool of host
// threads straight from float[3n] / uint64[k m], without a per-cell heap object in between.
#include "../../include/cuberille_hip.h"

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace {

inline char *put_float(char *p, float v) {
  if (std::isfinite(v)) {
    // == printf("%.9g", (double)v), which is what an ostream with precision(9) prints
    return std::to_chars(p, p + 32, v, std::chars_format::general, 9).ptr;
  }
  return p + std::snprintf(p, 32, "%.9g", (double)v);
}

inline char *put_u64(char *p, uint64_t v) { return std::to_chars(p, p + 24, v).ptr; }

void format_points(const float *pts, size_t i0, size_t i1, std::string &out) {
  out.resize((i1 - i0) * 3 * 20 + 16);
  char *p = &out[0];
  for (size_t i = i0; i < i1; i++) {
    p = put_float(p, pts[3 * i]);
    *p++ = ' ';
    p = put_float(p, pts[3 * i + 1]);
    *p++ = ' ';
    p = put_float(p, pts[3 * i + 2]);
    *p++ = '\n';
  }
  out.resize(p - &out[0]);
}

void format_cells(const uint64_t *cells, int k, size_t i0, size_t i1, std::string &out) {
  out.resize((i1 - i0) * (size_t)(k * 21 + 4) + 16);
  char *p = &out[0];
  for (size_t i = i0; i < i1; i++) {
    p = put_u64(p, (uint64_t)k);
    for (int j = 0; j < k; j++) {
      *p++ = ' ';
      p = put_u64(p, cells[i * k + j]);
    }
    *p++ = '\n';
  }
  out.resize(p - &out[0]);
}

// items [0,n) in rounds of T chunks: threads format, the caller's thread writes the chunks in order
template <class F> bool write_section(std::FILE *f, size_t n, int threads, F format) {
  const size_t chunk = 1u << 18;
  std::vector<std::string> buf(threads);
  for (size_t base = 0; base < n; base += chunk * threads) {
    std::vector<std::thread> pool;
    int used = 0;
    for (int t = 0; t < threads; t++) {
      const size_t i0 = base + chunk * t, i1 = std::min(n, i0 + chunk);
      if (i0 >= n) break;
      used++;
      if (t == 0) continue;  // the calling thread takes chunk 0
      pool.emplace_back([&, t, i0, i1] { format(i0, i1, buf[t]); });
    }
    format(base, std::min(n, base + chunk), buf[0]);
    for (auto &th : pool) th.join();
    for (int t = 0; t < used; t++)
      if (std::fwrite(buf[t].data(), 1, buf[t].size(), f) != buf[t].size()) return false;
  }
  return true;
}

}  // namespace

extern "C" int cuberille_write_vtk_buffers(const char *path, const float *points, uint64_t n_points,
                                           const uint64_t *cells, uint64_t n_cells, int verts_per_cell,
                                           int n_threads) {
  if (!path || (n_points && !points) || (n_cells && !cells)) return CUBERILLE_ERR_ARGUMENT;
  if (n_cells && verts_per_cell != 3 && verts_per_cell != 4) return CUBERILLE_ERR_ARGUMENT;
  if (n_threads <= 0) n_threads = (int)std::min(32u, std::max(1u, std::thread::hardware_concurrency()));
  std::FILE *f = std::fopen(path, "wb");
  if (!f) return CUBERILLE_ERR_ARGUMENT;
  std::vector<char> iobuf(8u << 20);
  std::setvbuf(f, iobuf.data(), _IOFBF, iobuf.size());
  bool ok = std::fprintf(f, "# vtk DataFile Version 2.0\nFile written by itkVTKPolyDataWriter\nASCII\nDATASET POLYDATA\n"
                            "POINTS %llu float\n", (unsigned long long)n_points) > 0;
  ok = ok && write_section(f, n_points, n_threads,
                           [&](size_t a, size_t b, std::string &s) { format_points(points, a, b, s); });
  ok = ok && std::fprintf(f, "POLYGONS %llu %llu\n", (unsigned long long)n_cells,
                          (unsigned long long)(n_cells * (uint64_t)(verts_per_cell + 1))) > 0;
  ok = ok && write_section(f, n_cells, n_threads, [&](size_t a, size_t b, std::string &s) {
         format_cells(cells, verts_per_cell, a, b, s);
       });
  ok = (std::fclose(f) == 0) && ok;
  return ok ? CUBERILLE_OK : CUBERILLE_ERR_STATE;
}

// cuberille_mesh_write_vtk on a context that holds point normals (cuberille_set_point_normals): the legacy format's point
// attribute block behind the polygons of a file cuberille_write_vtk_buffers has just written -- "POINT_DATA n",
// "NORMALS normals float", then "x y z" per point in the points' own number format.
namespace cuberille {
int append_vtk_normals(const char *path, const float *normals, uint64_t n_points, int n_threads) {
  if (!path || (n_points && !normals)) return CUBERILLE_ERR_ARGUMENT;
  if (n_threads <= 0) n_threads = (int)std::min(32u, std::max(1u, std::thread::hardware_concurrency()));
  std::FILE *f = std::fopen(path, "ab");
  if (!f) return CUBERILLE_ERR_ARGUMENT;
  bool ok = std::fprintf(f, "POINT_DATA %llu\nNORMALS normals float\n", (unsigned long long)n_points) > 0;
  ok = ok && write_section(f, n_points, n_threads,
                           [&](size_t a, size_t b, std::string &s) { format_points(normals, a, b, s); });
  ok = (std::fclose(f) == 0) && ok;
  return ok ? CUBERILLE_OK : CUBERILLE_ERR_STATE;
}

// ... and on one that holds cell pixels (cuberille_set_cell_pixels): the cell attribute block, LAST in the file (behind the
// normals where there are any, so that a file with normals alone stays what it was) -- "CELL_DATA n", "SCALARS pixel <type> 1",
// "LOOKUP_TABLE default", then one value per line: integers in decimal, float32 / float64 with the digits that read back to the
// same value (%.9g / %.17g).
int append_vtk_cell_pixels(const char *path, const void *pixels, int pixel_type, uint64_t n_cells) {
  if (!path || (n_cells && !pixels)) return CUBERILLE_ERR_ARGUMENT;
  const char *name = nullptr;
  switch (pixel_type) {
    case CUBERILLE_PIX_U8: name = "unsigned_char"; break;
    case CUBERILLE_PIX_I8: name = "char"; break;
    case CUBERILLE_PIX_U16: name = "unsigned_short"; break;
    case CUBERILLE_PIX_I16: name = "short"; break;
    case CUBERILLE_PIX_U32: name = "unsigned_int"; break;
    case CUBERILLE_PIX_I32: name = "int"; break;
    case CUBERILLE_PIX_F32: name = "float"; break;
    case CUBERILLE_PIX_F64: name = "double"; break;
    case CUBERILLE_PIX_I64: name = "vtktypeint64"; break;
    case CUBERILLE_PIX_U64: name = "vtktypeuint64"; break;
    default: return CUBERILLE_ERR_ARGUMENT;
  }
  std::FILE *f = std::fopen(path, "ab");
  if (!f) return CUBERILLE_ERR_ARGUMENT;
  bool ok = std::fprintf(f, "CELL_DATA %llu\nSCALARS pixel %s 1\nLOOKUP_TABLE default\n", (unsigned long long)n_cells, name) > 0;
  auto value = [&](char *p, size_t i) -> char * {
    switch (pixel_type) {
      case CUBERILLE_PIX_U8: return put_u64(p, ((const uint8_t *)pixels)[i]);
      case CUBERILLE_PIX_I8: return std::to_chars(p, p + 24, (long long)((const int8_t *)pixels)[i]).ptr;
      case CUBERILLE_PIX_U16: return put_u64(p, ((const uint16_t *)pixels)[i]);
      case CUBERILLE_PIX_I16: return std::to_chars(p, p + 24, (long long)((const int16_t *)pixels)[i]).ptr;
      case CUBERILLE_PIX_U32: return put_u64(p, ((const uint32_t *)pixels)[i]);
      case CUBERILLE_PIX_I32: return std::to_chars(p, p + 24, (long long)((const int32_t *)pixels)[i]).ptr;
      case CUBERILLE_PIX_F32: return put_float(p, ((const float *)pixels)[i]);
      case CUBERILLE_PIX_F64: return p + std::snprintf(p, 40, "%.17g", ((const double *)pixels)[i]);
      case CUBERILLE_PIX_I64: return std::to_chars(p, p + 24, (long long)((const int64_t *)pixels)[i]).ptr;
      default: return put_u64(p, ((const uint64_t *)pixels)[i]);
    }
  };
  std::string buf;
  const size_t chunk = 1u << 16;
  for (size_t i0 = 0; ok && i0 < n_cells; i0 += chunk) {
    const size_t i1 = std::min<size_t>(n_cells, i0 + chunk);
    buf.resize((i1 - i0) * 41 + 16);
    char *p = &buf[0];
    for (size_t i = i0; i < i1; i++) {
      p = value(p, i);
      *p++ = '\n';
    }
    const size_t n = (size_t)(p - &buf[0]);
    ok = std::fwrite(buf.data(), 1, n, f) == n;
  }
  ok = (std::fclose(f) == 0) && ok;
  return ok ? CUBERILLE_OK : CUBERILLE_ERR_STATE;
}

// ... and on one that holds components (cuberille_set_components): "SCALARS component unsigned_int 1", "LOOKUP_TABLE default",
// one label per line -- once in the point attribute block behind the normals, once in the cell attribute block behind the cell
// pixels.  block: "POINT_DATA" / "CELL_DATA" where this array is the block's first and opens it, null where the block exists.
int append_vtk_components(const char *path, const char *block, const uint32_t *labels, uint64_t n) {
  if (!path || (n && !labels)) return CUBERILLE_ERR_ARGUMENT;
  std::FILE *f = std::fopen(path, "ab");
  if (!f) return CUBERILLE_ERR_ARGUMENT;
  bool ok = true;
  if (block) ok = std::fprintf(f, "%s %llu\n", block, (unsigned long long)n) > 0;
  ok = ok && std::fprintf(f, "SCALARS component unsigned_int 1\nLOOKUP_TABLE default\n") > 0;
  std::string buf;
  const size_t chunk = 1u << 16;
  for (size_t i0 = 0; ok && i0 < n; i0 += chunk) {
    const size_t i1 = std::min<size_t>(n, i0 + chunk);
    buf.resize((i1 - i0) * 11 + 16);               // (a uint32 takes at most 10 digits)
    char *p = &buf[0];
    for (size_t i = i0; i < i1; i++) {
      p = put_u64(p, labels[i]);
      *p++ = '\n';
    }
    const size_t len = (size_t)(p - &buf[0]);
    ok = std::fwrite(buf.data(), 1, len, f) == len;
  }
  ok = (std::fclose(f) == 0) && ok;
  return ok ? CUBERILLE_OK : CUBERILLE_ERR_STATE;
}

// The point scalars' array of the POINT_DATA block (cuberille_set_point_scalars): one double per line as %.17g, which reads
// back to the same value (a NaN as "nan" or "-nan": its payload is not a text's to keep).
int append_vtk_point_scalars(const char *path, const char *block, const double *values, uint64_t n) {
  if (!path || (n && !values)) return CUBERILLE_ERR_ARGUMENT;
  std::FILE *f = std::fopen(path, "ab");
  if (!f) return CUBERILLE_ERR_ARGUMENT;
  bool ok = true;
  if (block) ok = std::fprintf(f, "%s %llu\n", block, (unsigned long long)n) > 0;
  ok = ok && std::fprintf(f, "SCALARS point_scalar double 1\nLOOKUP_TABLE default\n") > 0;
  for (uint64_t i = 0; ok && i < n; i++) ok = std::fprintf(f, "%.17g\n", values[i]) > 0;
  ok = (std::fclose(f) == 0) && ok;
  return ok ? CUBERILLE_OK : CUBERILLE_ERR_STATE;
}
}  // namespace cuberille
