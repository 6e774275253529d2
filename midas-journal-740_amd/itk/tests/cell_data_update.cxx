// SavePixelAsCellDataOn() of the drop-in, on an unsigned char label image and on a float image: (a) Update() with the projection
// off, quads and the switch on -- GetCellPixels() and the mesh's cell data against the pixel at the voxel read off each quad's
// lattice corners on the host (the face centre +- half a voxel along the face's axis: exactly one of the two is an inside voxel
// of the image); (b) the same values with the projection and triangles on, cells 2k and 2k + 1 both carrying quad k's; (c) the
// switch off: the array is empty and the mesh has no cell-data container.  The images are made here: unit spacing, origin and
// start index zero, so a lattice corner c stands at the point c - 1/2.  Exits non-zero on a difference.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "itkImage.h"
#include "itkMesh.h"
#include "itkCuberilleImageToMeshFilter.h"

typedef itk::Mesh<float, 3> MeshType;

template <class TPixel> struct Volume
{
  int nx, ny, nz;
  const TPixel *v;
  bool Has(const long u[3]) const { return u[0] >= 0 && u[0] < nx && u[1] >= 0 && u[1] < ny && u[2] >= 0 && u[2] < nz; }
  TPixel At(const long u[3]) const { return v[(static_cast<size_t>(u[2]) * ny + u[1]) * nx + u[0]]; }
};

// the inside voxel of the quad whose four corners are p (points of an unprojected mesh); false when the corners are no lattice face
template <class TPixel> static bool VoxelOfQuad(const Volume<TPixel> &vol, TPixel iso, const MeshType::PointType p[4], TPixel &pixel)
{
  double c[3] = {0.0, 0.0, 0.0};
  int axis = -1;
  for (int k = 0; k < 3; k++)
    {
    bool flat = true;
    for (int i = 0; i < 4; i++) { c[k] += p[i][k] / 4.0; flat = flat && p[i][k] == p[0][k]; }
    if (flat) { if (axis >= 0) return false; axis = k; }
    }
  if (axis < 0) return false;
  long a[3], b[3];
  for (int k = 0; k < 3; k++) a[k] = b[k] = std::lround(c[k]);          // (across the face: centre of the voxels' shared face)
  a[axis] = std::lround(c[axis] - 0.5);
  b[axis] = std::lround(c[axis] + 0.5);
  const bool ina = vol.Has(a) && !(vol.At(a) < iso), inb = vol.Has(b) && !(vol.At(b) < iso);
  if (ina == inb) return false;
  pixel = ina ? vol.At(a) : vol.At(b);
  return true;
}

template <class TPixel> static bool SameBits(TPixel a, TPixel b) { return std::memcmp(&a, &b, sizeof(TPixel)) == 0; }

template <class TPixel> static bool Run(const char *name, typename itk::Image<TPixel, 3>::Pointer image, int nx, int ny, int nz, TPixel iso)
{
  typedef itk::Image<TPixel, 3> ImageType;
  typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType> FilterType;
  const Volume<TPixel> vol = {nx, ny, nz, image->GetBufferPointer()};
  typename FilterType::Pointer f = FilterType::New();
  f->SetInput(image);
  f->SetIsoSurfaceValue(iso);
  f->SetGenerateTriangleFaces(false);
  f->SetProjectVerticesToIsoSurface(false);
  f->SavePixelAsCellDataOn();
  f->Update();
  MeshType *mesh = f->GetOutput();
  const std::vector<TPixel> quadPixels = f->GetCellPixels();
  const size_t n = mesh->GetNumberOfCells();
  bool ok = n > 256 && quadPixels.size() == n && mesh->GetCellData() != 0 && mesh->GetCellData()->Size() == n;
  size_t wrong = 0;
  for (size_t id = 0; ok && id < n; id++)
    {
    MeshType::CellAutoPointer cell;
    MeshType::PointType p[4];
    if (!mesh->GetCell(id, cell) || cell->GetNumberOfPoints() != 4) { ok = false; break; }
    for (int i = 0; i < 4; i++) mesh->GetPoint(cell->PointIdsBegin()[i], &p[i]);
    TPixel want;
    float stored = 0.0f;
    if (!VoxelOfQuad(vol, iso, p, want) || !SameBits(want, quadPixels[id]) || !mesh->GetCellData(id, &stored) ||
        !SameBits(stored, static_cast<float>(want)))
      wrong++;
    }
  std::cout << name << ": " << n << " quads, " << wrong << " with another pixel than their voxel's\n";
  ok = ok && wrong == 0;

  // the projection and triangles on: the same values, twice each
  f->SetGenerateTriangleFaces(true);
  f->SetProjectVerticesToIsoSurface(true);
  f->Update();
  const std::vector<TPixel> &triPixels = f->GetCellPixels();
  bool same = triPixels.size() == 2 * n && mesh->GetNumberOfCells() == 2 * n && mesh->GetCellData() != 0 &&
              mesh->GetCellData()->Size() == 2 * n;
  for (size_t k = 0; same && k < n; k++)
    {
    float s0 = 0.0f, s1 = 0.0f;
    same = SameBits(triPixels[2 * k], quadPixels[k]) && SameBits(triPixels[2 * k + 1], quadPixels[k]) &&
           mesh->GetCellData(2 * k, &s0) && mesh->GetCellData(2 * k + 1, &s1) &&
           SameBits(s0, static_cast<float>(quadPixels[k])) && SameBits(s1, static_cast<float>(quadPixels[k]));
    }
  std::cout << name << ": projected triangles " << (same ? "carry their quad's pixel" : "DIFFERENT") << "\n";

  // the switch off
  f->SavePixelAsCellDataOff();
  f->Update();
  const bool off = f->GetCellPixels().empty() && mesh->GetCellData() == 0 && mesh->GetNumberOfCells() == 2 * n;
  std::cout << name << ": SavePixelAsCellDataOff " << (off ? "empty, no container" : "DIFFERENT") << "\n";
  return ok && same && off;
}

template <class TPixel> static typename itk::Image<TPixel, 3>::Pointer MakeImage(int nx, int ny, int nz)
{
  typedef itk::Image<TPixel, 3> ImageType;
  typename ImageType::Pointer image = ImageType::New();
  typename ImageType::RegionType region;
  typename ImageType::IndexType start;
  typename ImageType::SizeType size;
  start[0] = start[1] = start[2] = 0;
  size[0] = nx; size[1] = ny; size[2] = nz;
  region.SetIndex(start);
  region.SetSize(size);
  image->SetRegions(region);
  image->Allocate();
  return image;
}

int main()
{
  try
    {
    // labels 0 .. 5 in blocks of 3 x 2 x 2 voxels from a small generator; label 0 is the background, and the object touches the border
    const int nx = 37, ny = 11, nz = 9;
    itk::Image<unsigned char, 3>::Pointer labels = MakeImage<unsigned char>(nx, ny, nz);
    for (int z = 0; z < nz; z++)
      for (int y = 0; y < ny; y++)
        for (int x = 0; x < nx; x++)
          {
          unsigned int h = static_cast<unsigned int>((x / 3) * 73856093u) ^ static_cast<unsigned int>((y / 2) * 19349663u) ^
                           static_cast<unsigned int>((z / 2) * 83492791u);
          h = (h ^ (h >> 13)) * 0x5bd1e995u;
          labels->GetBufferPointer()[(static_cast<size_t>(z) * ny + y) * nx + x] = static_cast<unsigned char>((h >> 7) % 6u);
          }
    bool all = Run<unsigned char>("uchar labels", labels, nx, ny, nz, static_cast<unsigned char>(1));

    // a smooth float field: a ball with a ripple, every pixel its own value
    const int mx = 30, my = 26, mz = 22;
    itk::Image<float, 3>::Pointer field = MakeImage<float>(mx, my, mz);
    for (int z = 0; z < mz; z++)
      for (int y = 0; y < my; y++)
        for (int x = 0; x < mx; x++)
          {
          const double r = std::sqrt((x - mx * 0.49) * (x - mx * 0.49) + (y - my * 0.52) * (y - my * 0.52) + (z - mz * 0.47) * (z - mz * 0.47));
          field->GetBufferPointer()[(static_cast<size_t>(z) * my + y) * mx + x] =
            static_cast<float>(300.0 - 22.5 * r + 9.0 * std::sin(0.4 * x) * std::cos(0.3 * y + 0.2 * z));
          }
    all = Run<float>("float field", field, mx, my, mz, 120.5f) && all;
    std::cout << (all ? "identical" : "DIFFERENT") << "\n";
    return all ? 0 : 1;
    }
  catch (itk::ExceptionObject &e)
    {
    std::cerr << e.what() << "\n";
    return 3;
    }
}
