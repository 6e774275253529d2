// GenerateComponentsOn() of the drop-in, on an unsigned char image of two separate balls: (a) Update() with quads --
// GetNumberOfComponents() is 2, and GetPointComponents() / GetCellComponents() / GetComponentCellCounts() equal a host union-find
// over the cells of the filled itk::Mesh (two points are joined when one cell holds both; components numbered in the order of
// their smallest point id; a cell is of its first point's component); (b) the projection and triangles on: the same point
// labels, the counts doubled, and again the host union-find over the mesh's triangles; (c) the switch off: the vectors are empty
// and the number is 0.  Exits non-zero on a difference.
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "itkImage.h"
#include "itkMesh.h"
#include "itkCuberilleImageToMeshFilter.h"

typedef itk::Mesh<float, 3> MeshType;
typedef itk::Image<unsigned char, 3> ImageType;
typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType> FilterType;

struct Components
{
  std::vector<uint32_t> point, cell;
  std::vector<uint64_t> cells;
};

static uint32_t Find(std::vector<uint32_t> &parent, uint32_t x)
{
  while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
  return x;
}

// the definition, serially, from the mesh's own cells
static bool HostComponents(MeshType *mesh, Components &out)
{
  const size_t nPoints = mesh->GetNumberOfPoints(), nCells = mesh->GetNumberOfCells();
  std::vector<uint32_t> parent(nPoints), first(nCells);
  for (size_t p = 0; p < nPoints; p++) parent[p] = static_cast<uint32_t>(p);
  for (size_t id = 0; id < nCells; id++)
    {
    MeshType::CellAutoPointer cell;
    if (!mesh->GetCell(id, cell) || cell->GetNumberOfPoints() < 3) return false;
    first[id] = static_cast<uint32_t>(cell->PointIdsBegin()[0]);
    for (unsigned int i = 1; i < cell->GetNumberOfPoints(); i++)
      {
      uint32_t a = Find(parent, first[id]), b = Find(parent, static_cast<uint32_t>(cell->PointIdsBegin()[i]));
      if (a != b) { if (a < b) parent[b] = a; else parent[a] = b; }      // the smaller stays the root
      }
    }
  std::vector<uint32_t> number(nPoints, 0);
  uint32_t k = 0;
  for (size_t p = 0; p < nPoints; p++) if (parent[p] == p) number[p] = k++;   // roots are minima: in the order of the smallest id
  out.point.resize(nPoints);
  out.cell.resize(nCells);
  out.cells.assign(k, 0);
  for (size_t p = 0; p < nPoints; p++) out.point[p] = number[Find(parent, static_cast<uint32_t>(p))];
  for (size_t id = 0; id < nCells; id++) { out.cell[id] = out.point[first[id]]; out.cells[out.cell[id]]++; }
  return true;
}

static bool Same(const char *what, FilterType *f, MeshType *mesh)
{
  Components want;
  if (!HostComponents(mesh, want)) { std::cout << what << ": the mesh's cells cannot be read\n"; return false; }
  const bool same = f->GetPointComponents() == want.point && f->GetCellComponents() == want.cell &&
                    f->GetComponentCellCounts() == want.cells && f->GetNumberOfComponents() == want.cells.size();
  std::cout << what << ": " << mesh->GetNumberOfPoints() << " points, " << mesh->GetNumberOfCells() << " cells, "
            << f->GetNumberOfComponents() << " components (host union-find: " << want.cells.size() << ") "
            << (same ? "identical" : "DIFFERENT") << "\n";
  return same;
}

int main()
{
  try
    {
    // two balls of radius 7 and 5, their centres 20 voxels apart: two closed surfaces
    const int nx = 44, ny = 24, nz = 22;
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
          const int b = (x - 31) * (x - 31) + (y - 11) * (y - 11) + (z - 10) * (z - 10);
          image->GetBufferPointer()[(static_cast<size_t>(z) * ny + y) * nx + x] = (a <= 49 || b <= 25) ? 200 : 0;
          }

    FilterType::Pointer f = FilterType::New();
    f->SetInput(image);
    f->SetIsoSurfaceValue(100);
    f->SetGenerateTriangleFaces(false);
    f->SetProjectVerticesToIsoSurface(false);
    f->GenerateComponentsOn();
    f->Update();
    MeshType *mesh = f->GetOutput();
    bool ok = f->GetNumberOfComponents() == 2 && mesh->GetNumberOfCells() > 256;
    std::cout << "two balls: GetNumberOfComponents() = " << f->GetNumberOfComponents() << "\n";
    ok = Same("quads", f.GetPointer(), mesh) && ok;
    const std::vector<uint32_t> quadPoints = f->GetPointComponents();
    const std::vector<uint64_t> quadCounts = f->GetComponentCellCounts();

    // the projection and triangles on: the same point labels, the counts doubled
    f->SetGenerateTriangleFaces(true);
    f->SetProjectVerticesToIsoSurface(true);
    f->Update();
    bool tri = Same("projected triangles", f.GetPointer(), mesh) && f->GetPointComponents() == quadPoints &&
               f->GetComponentCellCounts().size() == quadCounts.size();
    for (size_t k = 0; tri && k < quadCounts.size(); k++) tri = f->GetComponentCellCounts()[k] == 2 * quadCounts[k];
    std::cout << "projected triangles: " << (tri ? "the quads' point labels, the counts doubled" : "DIFFERENT") << "\n";

    // the switch off
    f->GenerateComponentsOff();
    f->Update();
    const bool off = f->GetPointComponents().empty() && f->GetCellComponents().empty() && f->GetComponentCellCounts().empty() &&
                     f->GetNumberOfComponents() == 0;
    std::cout << "GenerateComponentsOff: " << (off ? "empty" : "DIFFERENT") << "\n";
    const bool all = ok && tri && off;
    std::cout << (all ? "identical" : "DIFFERENT") << "\n";
    return all ? 0 : 1;
    }
  catch (itk::ExceptionObject &e)
    {
    std::cerr << e.what() << "\n";
    return 3;
    }
}
