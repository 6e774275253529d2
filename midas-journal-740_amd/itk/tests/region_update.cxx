// A box of a larger image through the drop-in: (a) the caller's recipe so far -- copy the box into an image of its own whose
// region keeps the index (what itk::ExtractImageFilter / RegionOfInterestImageFilter make), then the filter -- against (b) the
// filter with SetExtractionRegion() on the big image, which uploads the box's rows straight from it and makes no copy.  The
// two itk::Mesh objects must be equal point bit for point bit and cell for cell; both times are printed, (a)'s with its host
// crop loop included.  Exits non-zero on a difference.
//   usage: region_update <image.mha> <iso> <index x> <index y> <index z> <size x> <size y> <size z> [triangles = 1] [input start x y z]
//          region_update --synthetic <n> <iso> <index x y z> <size x y z>     (a float sphere field of n^3 made in memory)
//          region_update --desc <nx> <ny> <nz> <start x> <start y> <start z> <index x> <index y> <index z> <size x> <size y> <size z>
//            (no GPU: the description the library derives for the box, against a hand-made cropped itk::Image; prints both)
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "itkImage.h"
#include "itkImageFileReader.h"
#include "itkMesh.h"
#include "itkCuberilleImageToMeshFilter.h"

typedef itk::Image<float, 3> ImageType;
typedef itk::Mesh<float, 3> MeshType;
typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType> FilterType;

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

// the box of `big` as an image of its own: its region keeps the index, origin / spacing / direction are the big image's
static ImageType::Pointer Crop(const ImageType *big, const ImageType::RegionType &box)
{
  ImageType::Pointer out = ImageType::New();
  out->SetRegions(box);
  out->SetSpacing(big->GetSpacing());
  out->SetOrigin(big->GetOrigin());
  out->SetDirection(big->GetDirection());
  out->Allocate();
  const ImageType::RegionType &r = big->GetBufferedRegion();
  const long x0 = box.GetIndex()[0] - r.GetIndex()[0], y0 = box.GetIndex()[1] - r.GetIndex()[1], z0 = box.GetIndex()[2] - r.GetIndex()[2];
  const unsigned long Nx = r.GetSize()[0], Ny = r.GetSize()[1];
  const unsigned long nx = box.GetSize()[0], ny = box.GetSize()[1], nz = box.GetSize()[2];
  const float *src = big->GetBufferPointer();
  float *dst = out->GetBufferPointer();
  for (unsigned long z = 0; z < nz; z++)
    for (unsigned long y = 0; y < ny; y++)
      std::memcpy(dst + (z * ny + y) * nx, src + ((z0 + z) * Ny + (y0 + y)) * Nx + x0, nx * sizeof(float));
  return out;
}

static void Print(const char *who, const cuberille_image_desc &d)
{
  std::cout << who << " dims " << d.dims[0] << " " << d.dims[1] << " " << d.dims[2] << " start " << d.index_start[0] << " "
            << d.index_start[1] << " " << d.index_start[2] << " origin " << d.origin[0] << " " << d.origin[1] << " " << d.origin[2]
            << " spacing " << d.spacing[0] << " " << d.spacing[1] << " " << d.spacing[2] << "\n";
}

// no GPU: the library's description of the box against DescribeImage of a hand-made crop
static int DescOnly(char **a)
{
  ImageType::Pointer big = ImageType::New();
  ImageType::RegionType region, box;
  ImageType::IndexType start, index;
  ImageType::SizeType size, bsize;
  for (int i = 0; i < 3; i++)
    {
    size[i] = std::atol(a[i]); start[i] = std::atol(a[3 + i]);
    index[i] = std::atol(a[6 + i]); bsize[i] = std::atol(a[9 + i]);
    }
  region.SetIndex(start); region.SetSize(size);
  box.SetIndex(index); box.SetSize(bsize);
  big->SetRegions(region);
  ImageType::SpacingType sp; sp[0] = 0.7; sp[1] = 0.7; sp[2] = 2.5;
  ImageType::PointType org; org[0] = -3.0; org[1] = 4.5; org[2] = 10.0;
  big->SetSpacing(sp);
  big->SetOrigin(org);
  big->Allocate();
  const unsigned long n = region.GetNumberOfPixels();
  for (unsigned long i = 0; i < n; i++) big->GetBufferPointer()[i] = static_cast<float>(i % 97 + 1);
  cuberille_image_desc whole, derived, made;
  itk::cuberille_detail::DescribeImage(big.GetPointer(), whole);
  int64_t bstart[3], bsz[3];
  for (int i = 0; i < 3; i++) { bstart[i] = index[i] - start[i]; bsz[i] = static_cast<int64_t>(bsize[i]); }
  const int rc = cuberille_region_desc(&whole, bstart, bsz, &derived);
  if (rc != CUBERILLE_OK)
    {
    std::cout << "refused " << rc << "\n";
    return 0;
    }
  ImageType::Pointer crop = Crop(big, box);
  itk::cuberille_detail::DescribeImage(crop.GetPointer(), made);
  Print("library", derived);
  Print("crop   ", made);
  // ... and the crop's pixels are the big image's at the box's positions (the index arithmetic of the filter)
  bool same = derived.pixel_type == made.pixel_type;     // (field by field: the struct has padding)
  for (int i = 0; i < 3; i++)
    same = same && derived.dims[i] == made.dims[i] && derived.index_start[i] == made.index_start[i] &&
           derived.spacing[i] == made.spacing[i] && derived.origin[i] == made.origin[i];
  for (int i = 0; i < 9; i++) same = same && derived.direction[i] == made.direction[i];
  const unsigned long Nx = size[0], Ny = size[1];
  for (unsigned long z = 0; z < bsize[2] && same; z++)
    for (unsigned long y = 0; y < bsize[1] && same; y++)
      for (unsigned long x = 0; x < bsize[0]; x++)
        if (crop->GetBufferPointer()[(z * bsize[1] + y) * bsize[0] + x] !=
            big->GetBufferPointer()[((bstart[2] + z) * Ny + (bstart[1] + y)) * Nx + bstart[0] + x]) same = false;
  std::cout << (same ? "identical" : "DIFFERENT") << "\n";
  return same ? 0 : 1;
}

int main(int argc, char **argv)
{
  if (argc >= 14 && std::string(argv[1]) == "--desc") return DescOnly(argv + 2);
  const bool synthetic = argc >= 10 && std::string(argv[1]) == "--synthetic";
  if (argc < 9)
    {
    std::cerr << "usage: region_update <image.mha> <iso> <index xyz> <size xyz> [triangles] [input start xyz]\n";
    return 2;
    }
  const int base = synthetic ? 3 : 2;
  const float iso = static_cast<float>(std::atof(argv[base]));
  const bool triangles = !synthetic && argc > 9 ? std::atoi(argv[9]) != 0 : true;
  try
    {
    ImageType::Pointer image;
    if (synthetic)
      {
      const long n = std::atol(argv[2]);
      image = ImageType::New();
      ImageType::RegionType region;
      ImageType::IndexType start; start.Fill(0);
      ImageType::SizeType size; size.Fill(n);
      region.SetIndex(start); region.SetSize(size);
      image->SetRegions(region);
      image->Allocate();
      // concentric shells: surface everywhere in the volume, so that every box cuts it
      float *p = image->GetBufferPointer();
      const float c = 0.5f * (n - 1);
      for (long z = 0; z < n; z++)
        for (long y = 0; y < n; y++)
          for (long x = 0; x < n; x++)
            p[(z * n + y) * n + x] = 0.5f + 0.5f * std::sin(0.05f * std::sqrt((x - c) * (x - c) + (y - c) * (y - c) + (z - c) * (z - c)));
      }
    else
      {
      itk::ImageFileReader<ImageType>::Pointer reader = itk::ImageFileReader<ImageType>::New();
      reader->SetFileName(argv[1]);
      reader->Update();
      image = reader->GetOutput();
      image->DisconnectPipeline();
      if (argc > 12)
        {
        ImageType::RegionType r = image->GetBufferedRegion();
        ImageType::IndexType s;
        for (int i = 0; i < 3; i++) s[i] = std::atol(argv[10 + i]);
        r.SetIndex(s);
        image->SetRegions(r);      // (the buffer stays: only the region's index changes)
        }
      }
    ImageType::RegionType box;
    ImageType::IndexType index;
    ImageType::SizeType bsize;
    for (int i = 0; i < 3; i++) { index[i] = std::atol(argv[base + 1 + i]); bsize[i] = std::atol(argv[base + 4 + i]); }
    box.SetIndex(index); box.SetSize(bsize);

    // (a) crop on the host, then the filter
    FilterType::Pointer a = FilterType::New();
    a->SetIsoSurfaceValue(iso);
    a->SetGenerateTriangleFaces(triangles);
    ImageType::Pointer crop = Crop(image, box);
    a->SetInput(crop);
    a->Update();                       // (the first one of a filter sets up its workspace)
    double t0 = now();
    crop = Crop(image, box);
    const double cropSeconds = now() - t0;
    a->SetInput(crop);
    a->Modified();
    t0 = now();
    a->Update();
    const double aSeconds = now() - t0;

    // (b) the box in place
    FilterType::Pointer b = FilterType::New();
    b->SetExtractionRegion(box);
    b->SetInput(image);
    b->SetIsoSurfaceValue(iso);
    b->SetGenerateTriangleFaces(triangles);
    b->Update();
    b->Modified();
    t0 = now();
    b->Update();
    const double bSeconds = now() - t0;

    const bool same = SameMesh(a->GetOutput(), b->GetOutput());
    std::cout << "host crop " << cropSeconds * 1e3 << " ms + Update " << aSeconds * 1e3 << " ms (extract " << a->GetLastExtractSeconds() * 1e3
              << " ms); SetExtractionRegion Update " << bSeconds * 1e3 << " ms (extract " << b->GetLastExtractSeconds() * 1e3 << " ms); "
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
