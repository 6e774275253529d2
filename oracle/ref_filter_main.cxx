// ref_filter_main.cxx -- TEST INFRASTRUCTURE ONLY.  A driver of our own around the REFERENCE's own filter text:
// "itkCuberilleImageToMeshFilter.h" below resolves, through the -I the recipe gives (oracle/Makefile, target `ref`), to the
// reference's Source/ directory, and its GenerateData() is compiled unchanged against ITK-lite's host section
// (itk_lite/itkLiteHostFilter.h).  Nothing of the reference is in this file.
//
//   ref_filter <case file> <output file>
//
// case file: text lines `key value...` up to a line `end`, then raw little-endian voxels, x fastest: the FIRST image's
// (only with `first 1`), then the image's.
//   pixel     u8 i8 u16 i16 u32 i32 f32 f64 i64 u64          (the numbering of CUBERILLE_PIX_*)
//   interp    linear | bspline_f | bspline_d                  (TInterpolator: LinearInterpolateImageFunction<Image>, or
//             BSplineInterpolateImageFunction<Image,float,float> / <Image,double,double> with SetSplineOrder(3), as the
//             reference's driver writes it)
//   dims, spacing, origin, direction (9, row-major), start    the image; first_dims ... first_start the first image
//   iso       a double (C99 hex floats welcome), cast to the pixel type as the reference's driver casts its own
//   iso_int   instead, for the 64-bit integer types: the iso value itself
//   triangles, project, threshold, relax, max_steps           the setters the reference's driver calls
//   step      the same; a negative value is NOT set, so the constructor's -1 stays (the setter clamps to [0, 100000])
//   first 1   one filter object, Update() on the first image, SetInput(image), Update() again (quirk Q3)
//   pad 1     itk::ConstantPadImageFilter by one pixel of zero on every side first (the class comment's recipe)
// output file: uint64 points, uint64 cells, uint64 ids per cell, then float32 xyz per point and uint64 ids per cell, in
// identifier order.  The mesh is itk::Mesh<Pixel,3> as in the reference's driver: coordinates are float.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <stdint.h>
#include <string>
#include <vector>

#include "itkImage.h"
#include "itkMesh.h"
#include "itkCuberilleImageToMeshFilter.h"
#include "itkLinearInterpolateImageFunction.h"
#include "itkBSplineInterpolateImageFunction.h"
#include "itkConstantPadImageFilter.h"

namespace {

typedef std::map<std::string, std::vector<std::string> > Case;

double number(const Case &c, const std::string &key, size_t i = 0) {
  Case::const_iterator it = c.find(key);
  if (it == c.end() || it->second.size() <= i) { std::cerr << "case file: no " << key << "[" << i << "]\n"; std::exit(2); }
  return std::strtod(it->second[i].c_str(), 0);
}
long long integer(const Case &c, const std::string &key, size_t i = 0) {
  Case::const_iterator it = c.find(key);
  if (it == c.end() || it->second.size() <= i) { std::cerr << "case file: no " << key << "[" << i << "]\n"; std::exit(2); }
  return std::strtoll(it->second[i].c_str(), 0, 10);
}
bool has(const Case &c, const std::string &key) { return c.find(key) != c.end(); }

template <class TImage> typename TImage::Pointer read_image(const Case &c, const std::string &prefix, std::istream &in) {
  typename TImage::Pointer image = TImage::New();
  typename TImage::RegionType region;
  typename TImage::IndexType start;
  typename TImage::SizeType size;
  typename TImage::SpacingType spacing;
  typename TImage::PointType origin;
  typename TImage::DirectionType direction;
  for (unsigned int k = 0; k < 3; k++) {
    size[k] = static_cast<unsigned long>(integer(c, prefix + "dims", k));
    start[k] = static_cast<long>(integer(c, prefix + "start", k));
    spacing[k] = number(c, prefix + "spacing", k);
    origin[k] = number(c, prefix + "origin", k);
    for (unsigned int j = 0; j < 3; j++) direction[k][j] = number(c, prefix + "direction", k * 3 + j);
  }
  region.SetIndex(start);
  region.SetSize(size);
  image->SetRegions(region);
  image->SetSpacing(spacing);
  image->SetOrigin(origin);
  image->SetDirection(direction);
  image->Allocate();
  const size_t bytes = region.GetNumberOfPixels() * sizeof(typename TImage::PixelType);
  in.read(reinterpret_cast<char *>(image->GetBufferPointer()), static_cast<std::streamsize>(bytes));
  if (static_cast<size_t>(in.gcount()) != bytes) { std::cerr << "case file: voxels cut short\n"; std::exit(2); }
  return image;
}

template <class TInterpolator> void configure(TInterpolator *, int) {}
template <class TImage, class A, class B> void configure(itk::BSplineInterpolateImageFunction<TImage, A, B> *f, int) { f->SetSplineOrder(3); }

template <class TPixel, class TInterpolator> int run(const Case &c, std::istream &in, const char *outName) {
  typedef itk::Image<TPixel, 3> ImageType;
  typedef itk::Mesh<TPixel, 3> MeshType;
  typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType, TInterpolator> CuberilleType;
  typedef itk::ConstantPadImageFilter<ImageType, ImageType> PadType;

  typename ImageType::Pointer first;
  if (has(c, "first") && integer(c, "first")) first = read_image<ImageType>(c, "first_", in);
  typename ImageType::Pointer input = read_image<ImageType>(c, "", in);
  if (has(c, "pad") && integer(c, "pad")) {
    typename PadType::Pointer pad = PadType::New();
    typename ImageType::SizeType bound;
    bound.Fill(1);
    pad->SetInput(input);
    pad->SetPadBound(bound);
    pad->SetConstant(itk::NumericTraits<TPixel>::Zero);
    pad->Update();
    input = pad->GetOutput();
    input->DisconnectPipeline();
  }

  // (strtoull takes a minus sign and wraps: the same 64 bits either way)
  const TPixel iso = has(c, "iso_int") ? static_cast<TPixel>(std::strtoull(c.find("iso_int")->second[0].c_str(), 0, 10))
                                       : static_cast<TPixel>(number(c, "iso"));

  typename CuberilleType::Pointer cuberille = CuberilleType::New();
  cuberille->SetInput(first.IsNotNull() ? first : input);
  cuberille->SetIsoSurfaceValue(iso);
  typename TInterpolator::Pointer interpolator = TInterpolator::New();
  configure(interpolator.GetPointer(), 0);
  cuberille->SetInterpolator(interpolator);
  cuberille->SetGenerateTriangleFaces(integer(c, "triangles") != 0);
  cuberille->SetProjectVerticesToIsoSurface(integer(c, "project") != 0);
  cuberille->SetProjectVertexSurfaceDistanceThreshold(number(c, "threshold"));
  if (number(c, "step") >= 0.0) cuberille->SetProjectVertexStepLength(number(c, "step"));
  cuberille->SetProjectVertexStepLengthRelaxationFactor(number(c, "relax"));
  cuberille->SetProjectVertexMaximumNumberOfSteps(static_cast<unsigned int>(integer(c, "max_steps")));
  cuberille->Update();
  if (first.IsNotNull()) {
    cuberille->SetInput(input);
    cuberille->Update();
  }
  typename MeshType::Pointer mesh = cuberille->GetOutput();

  const uint64_t nPoints = mesh->GetNumberOfPoints(), nCells = mesh->GetNumberOfCells();
  uint64_t perCell = integer(c, "triangles") ? 3 : 4;
  std::vector<float> points(3 * nPoints);
  for (uint64_t i = 0; i < nPoints; i++) {
    typename MeshType::PointType p;
    mesh->GetPoint(i, &p);
    for (int k = 0; k < 3; k++) points[3 * i + k] = p[k];
  }
  std::vector<uint64_t> cells(perCell * nCells);
  for (uint64_t i = 0; i < nCells; i++) {
    typename MeshType::CellAutoPointer cell;
    mesh->GetCell(i, cell);
    if (cell->GetNumberOfPoints() != perCell) { std::cerr << "cell " << i << " has " << cell->GetNumberOfPoints() << " points\n"; return 3; }
    typename MeshType::CellType::PointIdConstIterator id = cell->PointIdsBegin();
    for (uint64_t k = 0; k < perCell; k++) cells[perCell * i + k] = id[k];
  }
  std::ofstream out(outName, std::ios::binary);
  const uint64_t head[3] = {nPoints, nCells, perCell};
  out.write(reinterpret_cast<const char *>(head), sizeof(head));
  out.write(reinterpret_cast<const char *>(points.data()), static_cast<std::streamsize>(points.size() * sizeof(float)));
  out.write(reinterpret_cast<const char *>(cells.data()), static_cast<std::streamsize>(cells.size() * sizeof(uint64_t)));
  out.close();
  return out ? 0 : 4;
}

template <class TPixel> int run_pixel(const Case &c, std::istream &in, const char *outName) {
  typedef itk::Image<TPixel, 3> ImageType;
  const std::string interp = has(c, "interp") ? c.find("interp")->second[0] : "linear";
  if (interp == "linear") return run<TPixel, itk::LinearInterpolateImageFunction<ImageType> >(c, in, outName);
  if (interp == "bspline_f") return run<TPixel, itk::BSplineInterpolateImageFunction<ImageType, float, float> >(c, in, outName);
  if (interp == "bspline_d") return run<TPixel, itk::BSplineInterpolateImageFunction<ImageType, double, double> >(c, in, outName);
  std::cerr << "case file: interp " << interp << "\n";
  return 2;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) { std::cerr << "usage: " << argv[0] << " <case file> <output file>\n"; return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  if (!in) { std::cerr << "cannot read " << argv[1] << "\n"; return 2; }
  Case c;
  std::string line;
  while (std::getline(in, line) && line != "end") {
    std::istringstream words(line);
    std::string key, word;
    words >> key;
    while (words >> word) c[key].push_back(word);
  }
  try {
    const std::string pixel = has(c, "pixel") ? c["pixel"][0] : "";
    if (pixel == "u8") return run_pixel<uint8_t>(c, in, argv[2]);
    if (pixel == "i8") return run_pixel<int8_t>(c, in, argv[2]);
    if (pixel == "u16") return run_pixel<uint16_t>(c, in, argv[2]);
    if (pixel == "i16") return run_pixel<int16_t>(c, in, argv[2]);
    if (pixel == "u32") return run_pixel<uint32_t>(c, in, argv[2]);
    if (pixel == "i32") return run_pixel<int32_t>(c, in, argv[2]);
    if (pixel == "f32") return run_pixel<float>(c, in, argv[2]);
    if (pixel == "f64") return run_pixel<double>(c, in, argv[2]);
    if (pixel == "i64") return run_pixel<int64_t>(c, in, argv[2]);
    if (pixel == "u64") return run_pixel<uint64_t>(c, in, argv[2]);
    std::cerr << "case file: pixel " << pixel << "\n";
    return 2;
  } catch (itk::ExceptionObject &e) {
    std::cerr << e << std::endl;
    return 1;
  }
}
