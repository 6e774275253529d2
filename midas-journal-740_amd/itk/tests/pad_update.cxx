// The reference's own recipe for an image whose surface meets the border (its class comment: pad the edges by at least one
// pixel with itk::ConstantPadImageFilter) against the drop-in's PadBorderOn(), which implies the same border without a
// padded copy: (a) pad filter -> cuberille filter, (b) cuberille filter with PadBorderOn() on the image as it is.  The two
// itk::Mesh objects must be equal point bit for point bit and cell for cell; both Update() times are printed, for (a) the
// pad filter's separately.  Exits non-zero on a difference.
//   usage: pad_update <image.mha> <iso> [pad value = 0] [triangles = 1]      (pixels are read as float)
//          pad_update --pad-only <int|float> <nx> <ny> <nz> <start x> <start y> <start z> <pad value>   (no GPU: the padded ramp image as text)
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "itkImage.h"
#include "itkImageFileReader.h"
#include "itkMesh.h"
#include "itkConstantPadImageFilter.h"
#include "itkCuberilleImageToMeshFilter.h"

typedef itk::Image<float, 3> ImageType;
typedef itk::Mesh<float, 3> MeshType;
typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType> FilterType;
typedef itk::ConstantPadImageFilter<ImageType, ImageType> PadType;

static double now()
{
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

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

// the pad filter alone on a ramp image with a start index of its own: region and every pixel of the output, as text
template <class TPixel> static int PadOnly(char **a)
{
  typedef itk::Image<TPixel, 3> Img;
  typename Img::Pointer in = Img::New();
  typename Img::RegionType region;
  typename Img::IndexType start;
  typename Img::SizeType size;
  for (int i = 0; i < 3; i++) { size[i] = std::atol(a[i]); start[i] = std::atol(a[3 + i]); }
  region.SetIndex(start);
  region.SetSize(size);
  in->SetRegions(region);
  in->Allocate();
  const unsigned long n = region.GetNumberOfPixels();
  for (unsigned long i = 0; i < n; i++) in->GetBufferPointer()[i] = static_cast<TPixel>(i % 97 + 1);
  typedef itk::ConstantPadImageFilter<Img, Img> Pad;
  typename Pad::Pointer pad = Pad::New();
  unsigned long one[3] = {1, 1, 1};
  pad->SetInput(in);
  pad->SetPadLowerBound(one);
  pad->SetPadUpperBound(one);
  pad->SetConstant(static_cast<TPixel>(std::atof(a[6])));
  pad->Update();
  const typename Img::RegionType &r = pad->GetOutput()->GetBufferedRegion();
  std::cout << "size " << r.GetSize()[0] << " " << r.GetSize()[1] << " " << r.GetSize()[2] << " start " << r.GetIndex()[0] << " "
            << r.GetIndex()[1] << " " << r.GetIndex()[2] << "\n";
  for (unsigned long i = 0; i < r.GetNumberOfPixels(); i++) std::cout << static_cast<double>(pad->GetOutput()->GetBufferPointer()[i]) << " ";
  std::cout << "\n";
  return 0;
}

int main(int argc, char **argv)
{
  if (argc >= 10 && std::string(argv[1]) == "--pad-only")
    return std::string(argv[2]) == "int" ? PadOnly<short>(argv + 3) : PadOnly<float>(argv + 3);
  if (argc < 3)
    {
    std::cerr << "usage: pad_update <image.mha> <iso> [pad value] [triangles]\n";
    return 2;
    }
  const float iso = static_cast<float>(std::atof(argv[2]));
  const float padValue = argc > 3 ? static_cast<float>(std::atof(argv[3])) : 0.0f;
  const bool triangles = argc > 4 ? std::atoi(argv[4]) != 0 : true;
  try
    {
    itk::ImageFileReader<ImageType>::Pointer reader = itk::ImageFileReader<ImageType>::New();
    reader->SetFileName(argv[1]);
    reader->Update();
    ImageType::Pointer image = reader->GetOutput();
    image->DisconnectPipeline();

    // (a) the reference's recipe
    PadType::Pointer pad = PadType::New();
    unsigned long one[3] = {1, 1, 1};
    pad->SetInput(image);
    pad->SetPadLowerBound(one);
    pad->SetPadUpperBound(one);
    pad->SetConstant(padValue);
    double t0 = now();
    pad->Update();
    const double padSeconds = now() - t0;
    ImageType::Pointer padded = pad->GetOutput();
    padded->DisconnectPipeline();
    FilterType::Pointer a = FilterType::New();
    a->SetInput(padded);
    a->SetIsoSurfaceValue(iso);
    a->SetGenerateTriangleFaces(triangles);
    a->Update();                       // (the first one of a filter sets up its workspace)
    a->Modified();
    t0 = now();
    a->Update();
    const double aSeconds = now() - t0;

    // (b) the implied border
    FilterType::Pointer b = FilterType::New();
    b->PadBorderOn();
    b->SetBorderPadValue(padValue);
    b->SetInput(image);
    b->SetIsoSurfaceValue(iso);
    b->SetGenerateTriangleFaces(triangles);
    b->Update();
    b->Modified();
    t0 = now();
    b->Update();
    const double bSeconds = now() - t0;

    const bool same = SameMesh(a->GetOutput(), b->GetOutput());
    std::cout << "pad filter " << padSeconds * 1e3 << " ms + Update " << aSeconds * 1e3 << " ms (extract " << a->GetLastExtractSeconds() * 1e3
              << " ms); PadBorderOn Update " << bSeconds * 1e3 << " ms (extract " << b->GetLastExtractSeconds() * 1e3 << " ms); "
              << b->GetOutput()->GetNumberOfPoints() << " points, " << b->GetOutput()->GetNumberOfCells() << " cells: "
              << (same ? "identical" : "DIFFERENT") << "\n";
    return same ? 0 : 1;
    }
  catch (itk::ExceptionObject &e)
    {
    std::cerr << e.what() << "\n";
    return 3;
    }
}
