// KeepLargestComponentOn() and SetMinimumComponentCells() of the drop-in, on an unsigned char image of two separate balls of
// different size (the small one holds the mesh's first points, so the largest component is not component 0): (a) the largest
// component kept -- the output mesh is exactly the mesh of the image with the small ball erased: the same points bit for bit,
// the same cells, the same cell data, and GetPointNormals() / GetCellPixels() / Get*Components() describe it, with quads and with
// projected triangles; (b) a minimum of cells between the two balls' sizes does the same; (c) a minimum above both yields an
// empty mesh without an exception; (d) both switches off: the mesh of the whole image again.  Exits non-zero on a difference.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "itkImage.h"
#include "itkMesh.h"
#include "itkCuberilleImageToMeshFilter.h"

typedef itk::Mesh<float, 3> MeshType;
typedef itk::Image<unsigned char, 3> ImageType;
typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType> FilterType;

static const int nx = 44, ny = 24, nz = 22;

// the large ball (radius 7, value 200) and, unless erased, the small one (radius 5, value 150), which starts three slices lower
static ImageType::Pointer TwoBalls(bool smallErased)
{
  ImageType::Pointer image = ImageType::New();
  ImageType::RegionType region;
  ImageType::IndexType start;
  ImageType::SizeType size;
  start[0] = start[1] = start[2] = 0;
  size[0] = nx; size[1] = ny; size[2] = nz;
  region.SetIndex(start);
  region.SetSize(size);
  image->SetRegions(region);
  image->Allocate();
  for (int z = 0; z < nz; z++)
    for (int y = 0; y < ny; y++)
      for (int x = 0; x < nx; x++)
        {
        const int a = (x - 11) * (x - 11) + (y - 12) * (y - 12) + (z - 11) * (z - 11);
        const int b = (x - 31) * (x - 31) + (y - 11) * (y - 11) + (z - 6) * (z - 6);
        image->GetBufferPointer()[(static_cast<size_t>(z) * ny + y) * nx + x] = a <= 49 ? 200 : (b <= 25 && !smallErased) ? 150 : 0;
        }
  return image;
}

// everything a caller can read of one Update()
struct Snapshot
{
  std::vector<float> points, normals;
  std::vector<uint64_t> cells;
  std::vector<float> cellData;
  std::vector<unsigned char> cellPixels;
  std::vector<uint32_t> pointComponents, cellComponents;
  std::vector<uint64_t> componentCells;
  bool readable;
};

static Snapshot Take(FilterType *f)
{
  Snapshot s;
  s.readable = true;
  MeshType *mesh = f->GetOutput();
  for (size_t p = 0; p < mesh->GetNumberOfPoints(); p++)
    {
    MeshType::PointType pt;
    if (!mesh->GetPoint(p, &pt)) s.readable = false;
    for (int i = 0; i < 3; i++) s.points.push_back(pt[i]);
    }
  for (size_t id = 0; id < mesh->GetNumberOfCells(); id++)
    {
    MeshType::CellAutoPointer cell;
    if (!mesh->GetCell(id, cell)) { s.readable = false; break; }
    s.cells.push_back(cell->GetNumberOfPoints());
    for (unsigned int i = 0; i < cell->GetNumberOfPoints(); i++) s.cells.push_back(cell->PointIdsBegin()[i]);
    MeshType::CellPixelType v = 0;
    if (mesh->GetCellData() != 0 && mesh->GetCellData(id, &v)) s.cellData.push_back(v);
    }
  s.normals = f->GetPointNormals();
  s.cellPixels = f->GetCellPixels();
  s.pointComponents = f->GetPointComponents();
  s.cellComponents = f->GetCellComponents();
  s.componentCells = f->GetComponentCellCounts();
  return s;
}

template <class T>
static bool SameBytes(const std::vector<T> &a, const std::vector<T> &b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(&a[0], &b[0], a.size() * sizeof(T)) == 0);
}

// the mesh and what belongs to it; the components of `got` are those of a mesh of one surface
static bool SameMesh(const char *what, const Snapshot &got, const Snapshot &want, size_t nPoints, size_t nCells)
{
  bool same = got.readable && want.readable && SameBytes(got.points, want.points) && SameBytes(got.cells, want.cells) &&
              SameBytes(got.cellData, want.cellData) && SameBytes(got.normals, want.normals) &&
              SameBytes(got.cellPixels, want.cellPixels);
  same = same && got.points.size() == 3 * nPoints && got.cellData.size() == nCells && got.cellPixels.size() == nCells &&
         got.normals.size() == 3 * nPoints;
  // one surface: every label 0, every cell in component 0
  same = same && got.pointComponents == std::vector<uint32_t>(nPoints, 0) && got.cellComponents == std::vector<uint32_t>(nCells, 0) &&
         got.componentCells == std::vector<uint64_t>(1, nCells);
  for (size_t i = 0; same && i < got.cellPixels.size(); i++) same = got.cellPixels[i] == 200;
  std::cout << what << ": " << nPoints << " points, " << nCells << " cells " << (same ? "identical" : "DIFFERENT") << "\n";
  return same;
}

static FilterType::Pointer Filter(ImageType *image, bool triangles)
{
  FilterType::Pointer f = FilterType::New();
  f->SetInput(image);
  f->SetIsoSurfaceValue(100);
  f->SetGenerateTriangleFaces(triangles);
  f->SetProjectVerticesToIsoSurface(triangles);
  f->GeneratePointNormalsOn();
  f->SavePixelAsCellDataOn();
  f->GenerateComponentsOn();
  return f;
}

int main()
{
  try
    {
    ImageType::Pointer both = TwoBalls(false), large = TwoBalls(true);
    bool all = true;
    for (int triangles = 0; triangles < 2; triangles++)
      {
      const char *kind = triangles ? "projected triangles" : "quads";
      // the mesh of the image with the small ball erased, and of the whole image
      FilterType::Pointer plain = Filter(large.GetPointer(), triangles != 0);
      plain->Update();
      const Snapshot want = Take(plain.GetPointer());
      const size_t nPoints = plain->GetOutput()->GetNumberOfPoints(), nCells = plain->GetOutput()->GetNumberOfCells();
      FilterType::Pointer f = Filter(both.GetPointer(), triangles != 0);
      f->Update();
      const Snapshot whole = Take(f.GetPointer());
      const std::vector<uint64_t> counts = f->GetComponentCellCounts();
      bool ok = counts.size() == 2 && counts[0] < counts[1] && counts[1] == nCells && nCells > 256 &&
                f->GetOutput()->GetNumberOfPoints() > nPoints;
      std::cout << kind << ": two balls of " << (counts.size() == 2 ? counts[0] : 0) << " and " << (counts.size() == 2 ? counts[1] : 0)
                << " cells, the largest is component 1: " << (ok ? "yes" : "NO") << "\n";
      if (!ok) { all = false; continue; }

      // (a) the largest component
      f->KeepLargestComponentOn();
      f->Update();
      all = SameMesh("KeepLargestComponentOn", Take(f.GetPointer()), want, nPoints, nCells) && f->GetNumberOfComponents() == 1 && all;
      // ... by itself: it turns the components on for its Update(), and they describe the kept mesh
      f->GenerateComponentsOff();
      f->Update();
      all = SameMesh("KeepLargestComponentOn alone", Take(f.GetPointer()), want, nPoints, nCells) && all;
      f->KeepLargestComponentOff();

      // (b) a minimum between the two sizes, and both switches together
      f->SetMinimumComponentCells(counts[0] + 1);
      f->Update();
      all = SameMesh("SetMinimumComponentCells between", Take(f.GetPointer()), want, nPoints, nCells) && all;
      f->KeepLargestComponentOn();
      f->Update();
      all = SameMesh("both switches", Take(f.GetPointer()), want, nPoints, nCells) && all;
      f->KeepLargestComponentOff();
      // ... at the small ball's size everything stays
      f->GenerateComponentsOn();
      f->SetMinimumComponentCells(counts[0]);
      f->Update();
      {
      const Snapshot kept = Take(f.GetPointer());
      const bool same = SameBytes(kept.points, whole.points) && SameBytes(kept.cells, whole.cells) &&
                        SameBytes(kept.cellData, whole.cellData) && kept.componentCells == counts;
      std::cout << "SetMinimumComponentCells at the small ball's size: " << (same ? "identical" : "DIFFERENT") << "\n";
      all = same && all;
      }

      // (c) above both: an empty mesh, no exception
      f->SetMinimumComponentCells(counts[1] + 1);
      f->Update();
      {
      const Snapshot none = Take(f.GetPointer());
      const bool empty = f->GetOutput()->GetNumberOfPoints() == 0 && f->GetOutput()->GetNumberOfCells() == 0 &&
                         f->GetNumberOfComponents() == 0 && none.normals.empty() && none.cellPixels.empty() &&
                         none.pointComponents.empty() && none.cellComponents.empty();
      std::cout << "SetMinimumComponentCells above both: " << (empty ? "empty, identical" : "DIFFERENT") << "\n";
      all = empty && all;
      }

      // (d) off again: the whole image's mesh
      f->SetMinimumComponentCells(0);
      f->Update();
      {
      const Snapshot back = Take(f.GetPointer());
      const bool same = SameBytes(back.points, whole.points) && SameBytes(back.cells, whole.cells) &&
                        SameBytes(back.cellData, whole.cellData) && back.componentCells == counts &&
                        SameBytes(back.pointComponents, whole.pointComponents);
      std::cout << "switches off: " << (same ? "identical" : "DIFFERENT") << "\n";
      all = same && all;
      }
      }
    std::cout << (all ? "keep_update ok" : "keep_update FAILED") << "\n";
    return all ? 0 : 1;
    }
  catch (itk::ExceptionObject &e)
    {
    std::cerr << e.what() << "\n";
    return 3;
    }
}
