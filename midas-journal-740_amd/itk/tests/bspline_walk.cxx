// The reference driver's B-spline configuration (Testing/CuberilleTest01.cxx with USE_BSPLINE_INTERPOLATOR:
// BSplineInterpolateImageFunction<ImageType, float, float>, SetSplineOrder(3)) as a driver of our own, plus the two
// pieces of that interpolator the tests hold to tests/bspline_ref.py.  Built with -ffp-contract=off (itk/Makefile).
//
//   bspline_walk coeffs <in.raw> <pixel> <nx> <ny> <nz> <coefBits> <out.raw> [order]
//       the interpolator's coefficient image (x fastest, coefBits wide); needs no GPU
//   bspline_walk eval <in.raw> <pixel> <nx> <ny> <nz> <coordBits> <coefBits> <geometry> <points.raw> <n> <out.raw> [order]
//       Evaluate() at n points (float64 xyz in, float64 values out); needs no GPU
//   bspline_walk walk <in.raw> <pixel> <nx> <ny> <nz> <bits> <geometry> <iso> <thr> <step> <relax> <maxSteps> <start.raw> <n> <out.raw>
//       the drop-in's host walk alone (HostGradient + HostWalk, what `filter ... host` runs after the device's sweep) through
//       BSplineInterpolateImageFunction<Image, T, T> of order 3: n start points (float32 xyz) -> walked points; needs no GPU
//       (<pixel>: all ten; the iso value travels as a double, so an 8-byte one must be one a double holds)
//   bspline_walk filter <volume> host|device <threads> <bits> <iso> <tri> <project> <thr> <step> <relax> <maxSteps>
//                <outPoints.raw> <outCells.raw> [raw <pixel> <nx> <ny> <nz>] [geometry <geometry>] [order <k>] [repeat <r>]
//       the whole filter with BSplineInterpolateImageFunction<Image, T, T> (T = float for 32, double for 64 bits): `host`
//       walks through the object on the host (SetBSplineOnDevice(false)) with <threads> threads, `device` on the GPU.
//       <volume> is a MetaImage, or a raw file described by `raw`.  `repeat`: Update() r times on the same filter (the later
//       ones warm: context, workspace and code objects set up).  Prints, for the last Update(), "<points> <cells> <update s>
//       <device s> <extract s> <download s> <mesh fill s>" (GetLastDeviceSeconds / -ExtractSeconds / -DownloadSeconds /
//       -MeshFillSeconds: the extract interval holds the upload and, on the host route, not the host walk).
//
// <pixel>: u8 i8 u16 i16 u32 i32 f32 f64 i64 u64 (filter: u8 i16 f32).  <geometry>: 18 comma-separated numbers -- spacing
// (3), origin (3), direction (9, row-major), region start index (3).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "itkImage.h"
#include "itkMesh.h"
#include "itkImageFileReader.h"
#include "itkBSplineInterpolateImageFunction.h"
#include "itkCuberilleImageToMeshFilter.h"

typedef itk::Mesh<float, 3> MeshType;

static void die(const char *what, const char *path)
{
  std::fprintf(stderr, "%s %s\n", what, path);
  std::exit(3);
}

static std::vector<char> slurp(const char *path, size_t bytes)
{
  std::vector<char> buf(bytes ? bytes : 1);
  FILE *f = std::fopen(path, "rb");
  if (!f || (bytes && std::fread(&buf[0], 1, bytes, f) != bytes)) die("cannot read", path);
  std::fclose(f);
  return buf;
}

static void dump(const char *path, const void *p, size_t bytes)
{
  FILE *f = std::fopen(path, "wb");
  if (!f || (bytes && std::fwrite(p, 1, bytes, f) != bytes)) die("cannot write", path);
  std::fclose(f);
}

struct Geometry
{
  double spacing[3], origin[3], direction[9];
  long start[3];
  bool given;
};

static Geometry parse_geometry(const char *s)
{
  Geometry g;
  double v[18];
  int n = 0;
  const char *p = s;
  while (n < 18 && *p)
    {
    char *end = 0;
    v[n++] = std::strtod(p, &end);
    p = (*end == ',') ? end + 1 : end;
    }
  if (n != 18) die("geometry needs 18 numbers:", s);
  for (int i = 0; i < 3; i++) { g.spacing[i] = v[i]; g.origin[i] = v[3 + i]; g.start[i] = (long)v[15 + i]; }
  for (int i = 0; i < 9; i++) g.direction[i] = v[6 + i];
  g.given = true;
  return g;
}

template <class TImage> void apply_geometry(TImage *image, const Geometry &g)
{
  if (!g.given) return;
  typename TImage::SpacingType sp;
  typename TImage::PointType org;
  typename TImage::DirectionType dir;
  for (int i = 0; i < 3; i++) { sp[i] = g.spacing[i]; org[i] = g.origin[i]; }
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) dir[r][c] = g.direction[r * 3 + c];
  image->SetSpacing(sp);
  image->SetOrigin(org);
  image->SetDirection(dir);
  typename TImage::RegionType region = image->GetBufferedRegion();
  typename TImage::IndexType start;
  for (int i = 0; i < 3; i++) start[i] = g.start[i];
  region.SetIndex(start);
  image->SetRegions(region);      // (the buffer stays: only the region's index changes)
}

template <class T> typename itk::Image<T, 3>::Pointer raw_image(const char *path, long nx, long ny, long nz)
{
  typedef itk::Image<T, 3> ImageType;
  typename ImageType::Pointer image = ImageType::New();
  typename ImageType::RegionType region;
  typename ImageType::IndexType start;
  typename ImageType::SizeType size;
  start.Fill(0);
  size[0] = nx; size[1] = ny; size[2] = nz;
  region.SetIndex(start);
  region.SetSize(size);
  image->SetRegions(region);
  image->Allocate();
  const size_t n = (size_t)nx * ny * nz;
  std::vector<char> buf = slurp(path, n * sizeof(T));
  std::memcpy(image->GetBufferPointer(), &buf[0], n * sizeof(T));
  return image;
}

template <class T, class C> int coeffs(char **argv, int argc)
{
  typedef itk::Image<T, 3> ImageType;
  typename ImageType::Pointer image = raw_image<T>(argv[2], std::atol(argv[4]), std::atol(argv[5]), std::atol(argv[6]));
  typedef itk::BSplineInterpolateImageFunction<ImageType, C, C> Interp;
  typename Interp::Pointer interp = Interp::New();
  interp->SetSplineOrder(argc > 9 ? (unsigned)std::atoi(argv[9]) : 3u);
  interp->SetInputImage(image);
  dump(argv[8], interp->GetCoefficients()->GetBufferPointer(), sizeof(C) * image->GetBufferedRegion().GetNumberOfPixels());
  return 0;
}

template <class T, class C> int eval(char **argv, int argc)
{
  typedef itk::Image<T, 3> ImageType;
  typename ImageType::Pointer image = raw_image<T>(argv[2], std::atol(argv[4]), std::atol(argv[5]), std::atol(argv[6]));
  apply_geometry(image.GetPointer(), parse_geometry(argv[9]));
  typedef itk::BSplineInterpolateImageFunction<ImageType, C, C> Interp;
  typename Interp::Pointer interp = Interp::New();
  interp->SetSplineOrder(argc > 13 ? (unsigned)std::atoi(argv[13]) : 3u);
  interp->SetInputImage(image);
  const size_t n = (size_t)std::atoll(argv[11]);
  std::vector<char> buf = slurp(argv[10], n * 3 * sizeof(double));
  const double *pts = reinterpret_cast<const double *>(&buf[0]);
  std::vector<double> out(n ? n : 1);
  for (size_t i = 0; i < n; i++)
    {
    typename Interp::PointType q;
    for (int k = 0; k < 3; k++) q[k] = static_cast<C>(pts[3 * i + k]);
    out[i] = interp->Evaluate(q);
    }
  dump(argv[12], &out[0], n * sizeof(double));
  return 0;
}

template <class T, class C> int walk(char **argv)
{
  typedef itk::Image<T, 3> ImageType;
  typename ImageType::Pointer image = raw_image<T>(argv[2], std::atol(argv[4]), std::atol(argv[5]), std::atol(argv[6]));
  apply_geometry(image.GetPointer(), parse_geometry(argv[8]));
  typedef itk::BSplineInterpolateImageFunction<ImageType, C, C> Interp;
  typename Interp::Pointer interp = Interp::New();
  interp->SetSplineOrder(3);
  interp->SetInputImage(image);
  const size_t n = (size_t)std::atoll(argv[15]);
  std::vector<char> buf = slurp(argv[14], n * 3 * sizeof(float));
  float *pts = reinterpret_cast<float *>(&buf[0]);
  itk::cuberille_detail::HostGradient<ImageType> gradient(image.GetPointer());
  itk::cuberille_detail::HostWalk<ImageType, Interp> w =
    {&gradient, interp.GetPointer(), pts, static_cast<double>(static_cast<T>(std::atof(argv[9]))), std::atof(argv[10]), std::atof(argv[11]),
     std::atof(argv[12]), (unsigned int)std::atoi(argv[13])};
  itk::cuberille_detail::ParallelRanges(n, w, 1u);
  dump(argv[16], pts, n * 3 * sizeof(float));
  return 0;
}

template <class T, class C> int filter(int argc, char **argv)
{
  typedef itk::Image<T, 3> ImageType;
  typename ImageType::Pointer image;
  Geometry geo;
  geo.given = false;
  unsigned int order = 3;
  int repeat = 1;
  const char *rawPixel = 0;
  long dims[3] = {0, 0, 0};
  for (int a = 15; a < argc; a++)
    {
    if (!std::strcmp(argv[a], "raw") && a + 4 < argc)
      { rawPixel = argv[a + 1]; for (int i = 0; i < 3; i++) dims[i] = std::atol(argv[a + 2 + i]); a += 4; }
    else if (!std::strcmp(argv[a], "geometry") && a + 1 < argc) geo = parse_geometry(argv[++a]);
    else if (!std::strcmp(argv[a], "order") && a + 1 < argc) order = (unsigned)std::atoi(argv[++a]);
    else if (!std::strcmp(argv[a], "repeat") && a + 1 < argc) repeat = std::atoi(argv[++a]);
    }
  if (rawPixel) image = raw_image<T>(argv[2], dims[0], dims[1], dims[2]);
  else
    {
    typedef itk::ImageFileReader<ImageType> ReaderType;
    typename ReaderType::Pointer reader = ReaderType::New();
    reader->SetFileName(argv[2]);
    reader->Update();
    image = reader->GetOutput();
    }
  apply_geometry(image.GetPointer(), geo);

  typedef itk::BSplineInterpolateImageFunction<ImageType, C, C> Interp;
  typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType, Interp> FilterType;
  typename Interp::Pointer interp = Interp::New();
  interp->SetSplineOrder(order);                              // (CuberilleTest01.cxx:150)
  typename FilterType::Pointer f = FilterType::New();
  f->SetInput(image);
  f->SetInterpolator(interp);
  f->SetBSplineOnDevice(std::strcmp(argv[3], "device") == 0);
  f->SetHostWalkThreads((unsigned int)std::atoi(argv[4]));
  f->SetIsoSurfaceValue(static_cast<T>(std::atof(argv[6])));
  f->SetGenerateTriangleFaces(std::atoi(argv[7]) != 0);
  f->SetProjectVerticesToIsoSurface(std::atoi(argv[8]) != 0);
  f->SetProjectVertexSurfaceDistanceThreshold(std::atof(argv[9]));
  f->SetProjectVertexStepLength(std::atof(argv[10]));
  f->SetProjectVertexStepLengthRelaxationFactor(std::atof(argv[11]));
  f->SetProjectVertexMaximumNumberOfSteps((unsigned int)std::atoi(argv[12]));
  double seconds = 0.0;
  for (int r = 0; r < (repeat > 0 ? repeat : 1); r++)
    {
    f->Modified();
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    f->Update();
    seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
  MeshType::Pointer mesh = f->GetOutput();
  std::vector<float> pts(3 * mesh->GetNumberOfPoints());
  for (unsigned long i = 0; i < mesh->GetNumberOfPoints(); i++)
    {
    MeshType::PointType p;
    mesh->GetPoint(i, &p);
    for (int k = 0; k < 3; k++) pts[3 * i + k] = p[k];
    }
  std::vector<unsigned long long> ids;
  for (unsigned long c = 0; c < mesh->GetNumberOfCells(); c++)
    {
    MeshType::CellAutoPointer cell;
    mesh->GetCell(c, cell);
    for (unsigned int k = 0; k < cell->GetNumberOfPoints(); k++) ids.push_back(cell->PointIdsBegin()[k]);
    }
  dump(argv[13], pts.empty() ? 0 : &pts[0], sizeof(float) * pts.size());
  dump(argv[14], ids.empty() ? 0 : &ids[0], sizeof(unsigned long long) * ids.size());
  std::cout << mesh->GetNumberOfPoints() << " " << mesh->GetNumberOfCells() << " " << seconds << " " << f->GetLastDeviceSeconds()
            << " " << f->GetLastExtractSeconds() << " " << f->GetLastDownloadSeconds() << " " << f->GetLastMeshFillSeconds()
            << std::endl;
  return 0;
}

template <class T> int by_bits(const char *mode, int bits, int argc, char **argv)
{
  if (!std::strcmp(mode, "coeffs")) return bits == 64 ? coeffs<T, double>(argv, argc) : coeffs<T, float>(argv, argc);
  return bits == 64 ? eval<T, double>(argv, argc) : eval<T, float>(argv, argc);
}

template <class T> int filter_bits(int bits, int argc, char **argv)
{
  return bits == 64 ? filter<T, double>(argc, argv) : filter<T, float>(argc, argv);
}

int main(int argc, char **argv)
{
  if (argc < 2) { std::fprintf(stderr, "usage: see the head of bspline_walk.cxx\n"); return 1; }
  const char *mode = argv[1];
  try
    {
    if (!std::strcmp(mode, "coeffs") || !std::strcmp(mode, "eval"))
      {
      if (argc < (!std::strcmp(mode, "coeffs") ? 9 : 13)) { std::fprintf(stderr, "too few arguments\n"); return 1; }
      const std::string px = argv[3];
      const int bits = std::atoi(argv[!std::strcmp(mode, "coeffs") ? 7 : 8]);
      if (!std::strcmp(mode, "eval") && std::atoi(argv[7]) != bits) { std::fprintf(stderr, "coordinate and coefficient bits differ\n"); return 1; }
      if (px == "u8") return by_bits<unsigned char>(mode, bits, argc, argv);
      if (px == "i8") return by_bits<signed char>(mode, bits, argc, argv);
      if (px == "u16") return by_bits<unsigned short>(mode, bits, argc, argv);
      if (px == "i16") return by_bits<short>(mode, bits, argc, argv);
      if (px == "u32") return by_bits<unsigned int>(mode, bits, argc, argv);
      if (px == "i32") return by_bits<int>(mode, bits, argc, argv);
      if (px == "f32") return by_bits<float>(mode, bits, argc, argv);
      if (px == "f64") return by_bits<double>(mode, bits, argc, argv);
      if (px == "i64") return by_bits<long long>(mode, bits, argc, argv);
      if (px == "u64") return by_bits<unsigned long long>(mode, bits, argc, argv);
      std::fprintf(stderr, "unknown pixel type %s\n", px.c_str());
      return 1;
      }
    if (!std::strcmp(mode, "walk"))
      {
      if (argc < 17) { std::fprintf(stderr, "too few arguments\n"); return 1; }
      const std::string px = argv[3];
      const bool wide = std::atoi(argv[7]) == 64;
      if (px == "u8") return wide ? walk<unsigned char, double>(argv) : walk<unsigned char, float>(argv);
      if (px == "i16") return wide ? walk<short, double>(argv) : walk<short, float>(argv);
      if (px == "f32") return wide ? walk<float, double>(argv) : walk<float, float>(argv);
      if (px == "i8") return wide ? walk<signed char, double>(argv) : walk<signed char, float>(argv);
      if (px == "u16") return wide ? walk<unsigned short, double>(argv) : walk<unsigned short, float>(argv);
      if (px == "u32") return wide ? walk<unsigned int, double>(argv) : walk<unsigned int, float>(argv);
      if (px == "i32") return wide ? walk<int, double>(argv) : walk<int, float>(argv);
      if (px == "f64") return wide ? walk<double, double>(argv) : walk<double, float>(argv);
      if (px == "i64") return wide ? walk<long long, double>(argv) : walk<long long, float>(argv);
      if (px == "u64") return wide ? walk<unsigned long long, double>(argv) : walk<unsigned long long, float>(argv);
      std::fprintf(stderr, "walk: unsupported pixel type %s\n", px.c_str());
      return 1;
      }
    if (!std::strcmp(mode, "filter"))
      {
      if (argc < 15) { std::fprintf(stderr, "too few arguments\n"); return 1; }
      const int bits = std::atoi(argv[5]);
      std::string px = "u8";
      for (int a = 15; a + 1 < argc; a++) if (!std::strcmp(argv[a], "raw")) px = argv[a + 1];
      if (px == "u8") return filter_bits<unsigned char>(bits, argc, argv);
      if (px == "i16") return filter_bits<short>(bits, argc, argv);
      if (px == "f32") return filter_bits<float>(bits, argc, argv);
      std::fprintf(stderr, "filter: unsupported pixel type %s\n", px.c_str());
      return 1;
      }
    std::fprintf(stderr, "unknown mode %s\n", mode);
    return 1;
    }
  catch (itk::ExceptionObject &e)
    {
    std::cerr << e << std::endl;
    return 2;
    }
}
