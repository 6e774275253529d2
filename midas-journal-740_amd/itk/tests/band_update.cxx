// The caller's recipe for one label or a value band (itk::BinaryThresholdImageFilter, then the filter -- the reference's own
// driver holds that filter ready) against the drop-in's InsideBandOn(), which implies the same binary image without a
// thresholded copy: (a) threshold filter -> cuberille filter, (b) cuberille filter with SetInsideBand / InsideBandOn on the
// image as it is.  The two itk::Mesh objects must be equal point bit for point bit and cell for cell, for the default band
// values (1 / 0, iso 1) and for 200 / 10 at iso 100; then InsideBandOff() on (b) and a second Update() against the plain
// filter on the image.  The image is made here: 96^3 nested-sphere labels 0 .. 4 (unsigned char), or a smooth float field.
// Exits non-zero on a difference.
//   usage: band_update <uchar|float> [triangles = 1]
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "itkImage.h"
#include "itkMesh.h"
#include "itkBinaryThresholdImageFilter.h"
#include "itkCuberilleImageToMeshFilter.h"

typedef itk::Mesh<float, 3> MeshType;

static bool SameMesh(const MeshType *a, const MeshType *b)
{
  if (a->GetNumberOfPoints() != b->GetNumberOfPoints() || a->GetNumberOfCells() != b->GetNumberOfCells()) return false;
  for (unsigned long i = 0; i < a->GetNumberOfPoints(); i++)
    {
    MeshType::PointType p, q;
    a->GetPoint(i, &p);
    b->GetPoint(i, &q);
    for (int k = 0; k < 3; k++)
      {
      const float x = p[k], y = q[k];
      if (std::memcmp(&x, &y, sizeof x) != 0) return false;
      }
    }
  for (unsigned long c = 0; c < a->GetNumberOfCells(); c++)
    {
    MeshType::CellAutoPointer ca, cb;
    if (!a->GetCell(c, ca) || !b->GetCell(c, cb)) return false;
    if (ca->GetNumberOfPoints() != cb->GetNumberOfPoints()) return false;
    MeshType::CellType::PointIdConstIterator i = ca->PointIdsBegin(), j = cb->PointIdsBegin();
    for (; i != ca->PointIdsEnd(); ++i, ++j)
      if (*i != *j) return false;
    }
  return true;
}

template <class TPixel> static int Run(bool labels, bool triangles)
{
  typedef itk::Image<TPixel, 3> ImageType;
  typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType> FilterType;
  typedef itk::BinaryThresholdImageFilter<ImageType, ImageType> ThresholdType;
  const int n = 96;
  typename ImageType::Pointer image = ImageType::New();
  typename ImageType::RegionType region;
  typename ImageType::IndexType start;
  typename ImageType::SizeType size;
  for (int i = 0; i < 3; i++) { start[i] = 3 * i - 2; size[i] = n; }
  region.SetIndex(start);
  region.SetSize(size);
  image->SetRegions(region);
  image->Allocate();
  typename ImageType::SpacingType spacing;
  spacing[0] = 0.7; spacing[1] = 0.7; spacing[2] = 2.5;
  image->SetSpacing(spacing);
  const double radii[4] = {0.45, 0.38, 0.27, 0.15};
  for (int z = 0; z < n; z++)
    for (int y = 0; y < n; y++)
      for (int x = 0; x < n; x++)
        {
        const double r = std::sqrt((x - n * 0.49) * (x - n * 0.49) + (y - n * 0.52) * (y - n * 0.52) + (z - n * 0.47) * (z - n * 0.47));
        double v;
        if (labels) { v = 0.0; for (int k = 0; k < 4; k++) v += r < n * radii[k] ? 1.0 : 0.0; }
        else v = 300.0 - 12.5 * r + 9.0 * std::sin(0.4 * x) * std::cos(0.3 * y + 0.2 * z);
        image->GetBufferPointer()[(static_cast<size_t>(z) * n + y) * n + x] = static_cast<TPixel>(v);
        }
  const TPixel lower = static_cast<TPixel>(labels ? 2 : -200.25), upper = static_cast<TPixel>(labels ? 3 : 120.5);
  const TPixel values[2][3] = {{static_cast<TPixel>(1), static_cast<TPixel>(0), static_cast<TPixel>(1)},
                               {static_cast<TPixel>(200), static_cast<TPixel>(10), static_cast<TPixel>(100)}};
  typename FilterType::Pointer b = FilterType::New();
  b->SetInput(image);
  b->SetGenerateTriangleFaces(triangles);
  bool all = true;
  for (int c = 0; c < 2; c++)
    {
    // (a) the recipe
    typename ThresholdType::Pointer threshold = ThresholdType::New();
    threshold->SetInput(image);
    threshold->SetLowerThreshold(lower);
    threshold->SetUpperThreshold(upper);
    threshold->SetInsideValue(values[c][0]);
    threshold->SetOutsideValue(values[c][1]);
    threshold->Update();
    typename FilterType::Pointer a = FilterType::New();
    a->SetInput(threshold->GetOutput());
    a->SetIsoSurfaceValue(values[c][2]);
    a->SetGenerateTriangleFaces(triangles);
    a->Update();
    // (b) the implied band
    b->SetInsideBand(lower, upper);
    if (c) b->SetBandValues(values[c][0], values[c][1]);
    b->InsideBandOn();
    b->SetIsoSurfaceValue(values[c][2]);
    b->Update();
    const bool same = SameMesh(a->GetOutput(), b->GetOutput()) && b->GetOutput()->GetNumberOfCells() > 1000;
    std::cout << "band values " << static_cast<double>(values[c][0]) << " / " << static_cast<double>(values[c][1]) << ": "
              << b->GetOutput()->GetNumberOfPoints() << " points, " << b->GetOutput()->GetNumberOfCells() << " cells: "
              << (same ? "same" : "DIFFERENT") << "\n";
    all = all && same;
    }
  // the way back: InsideBandOff() and a second Update() against the plain filter
  const TPixel iso = static_cast<TPixel>(labels ? 3 : 120.5);
  b->InsideBandOff();
  b->SetIsoSurfaceValue(iso);
  b->Update();
  typename FilterType::Pointer plain = FilterType::New();
  plain->SetInput(image);
  plain->SetIsoSurfaceValue(iso);
  plain->SetGenerateTriangleFaces(triangles);
  plain->Update();
  const bool back = SameMesh(plain->GetOutput(), b->GetOutput()) && b->GetOutput()->GetNumberOfCells() > 1000;
  std::cout << "InsideBandOff: " << b->GetOutput()->GetNumberOfCells() << " cells: " << (back ? "same" : "DIFFERENT") << "\n";
  // lower > upper: Update() throws, as the threshold filter does
  bool threw = false;
  b->SetInsideBand(upper, lower);
  b->InsideBandOn();
  try { b->Update(); } catch (itk::ExceptionObject &e) { threw = std::string(e.what()).find("band") != std::string::npos; }
  std::cout << "lower > upper: " << (threw ? "refused" : "NOT REFUSED") << "\n";
  all = all && back && threw;
  std::cout << (all ? "identical" : "DIFFERENT") << "\n";
  return all ? 0 : 1;
}

int main(int argc, char **argv)
{
  if (argc < 2)
    {
    std::cerr << "usage: band_update <uchar|float> [triangles]\n";
    return 2;
    }
  const bool triangles = argc > 2 ? std::atoi(argv[2]) != 0 : true;
  try
    {
    if (std::string(argv[1]) == "uchar") return Run<unsigned char>(true, triangles);
    return Run<float>(false, triangles);
    }
  catch (itk::ExceptionObject &e)
    {
    std::cerr << e.what() << "\n";
    return 3;
    }
}
