// One Update() of the drop-in filter split over a context group (SetDevices) against the same Update() on one context:
// runs both on an n^3 float sphere distance field, reports where the grouped Update() goes, and checks that the two
// output meshes are equal byte for byte (point coordinates as float bits, every cell's point ids, in order).
//   usage: multi_update <n> <devices> [triangles=1]      devices: ids separated by commas, e.g. 0,0 or 0,1,2,3
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "itkImage.h"
#include "itkMesh.h"
#include "itkCuberilleImageToMeshFilter.h"

typedef itk::Image<float, 3> ImageType;
typedef itk::Mesh<float, 3> MeshType;
typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType> FilterType;

static double now()
{
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Run
{
  MeshType::Pointer mesh;
  double update, extract, download, fill, device;
  unsigned int slabs;
};

// one filter, one warm Update() timed (the first one of a filter sets up its workspace)
static Run RunFilter(ImageType *image, const std::vector<int> &devices, bool triangles)
{
  FilterType::Pointer filter = FilterType::New();
  filter->SetDevices(devices);
  if (!devices.empty()) filter->SetDevice(devices[0]);
  filter->SetInput(image);
  filter->SetIsoSurfaceValue(0.0f);
  filter->SetGenerateTriangleFaces(triangles);
  filter->SetProjectVertexSurfaceDistanceThreshold(0.05);
  filter->SetProjectVertexStepLength(0.25);
  filter->Update();
  filter->Modified();
  const double t0 = now();
  filter->Update();
  Run r;
  r.update = now() - t0;
  r.extract = filter->GetLastExtractSeconds();
  r.download = filter->GetLastDownloadSeconds();
  r.fill = filter->GetLastMeshFillSeconds();
  r.device = filter->GetLastDeviceSeconds();
  r.slabs = filter->GetLastNumberOfSlabs();
  r.mesh = filter->GetOutput();
  r.mesh->DisconnectPipeline();
  return r;
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

int main(int argc, char *argv[])
{
  if (argc < 3) { std::cerr << "usage: multi_update <n> <devices> [triangles]" << std::endl; return 2; }
  const int n = std::atoi(argv[1]);
  std::vector<int> devices;
  if (!itk::cuberille_detail::ParseDeviceList(argv[2], devices))
    {
    std::cerr << "devices: ids separated by commas, e.g. 0,0" << std::endl;
    return 2;
    }
  const bool triangles = argc > 3 ? std::atoi(argv[3]) != 0 : true;
  try
    {
    ImageType::Pointer image = ImageType::New();
    ImageType::RegionType region;
    ImageType::IndexType start;
    ImageType::SizeType size;
    start.Fill(0);
    size.Fill(n);
    region.SetIndex(start);
    region.SetSize(size);
    image->SetRegions(region);
    image->Allocate();
    float *px = image->GetBufferPointer();
    const double c = 0.5 * (n - 1), R = 0.4 * n;
    for (int z = 0; z < n; z++)
      for (int y = 0; y < n; y++)
        for (int x = 0; x < n; x++)
          {
          const double dx = x - (c + 0.25), dy = y - (c + 0.125), dz = z - (c + 0.0625);
          px[((size_t)z * n + y) * n + x] = static_cast<float>(R - std::sqrt(dx * dx + dy * dy + dz * dz));
          }
    const Run split = RunFilter(image, devices, triangles);
    const Run one = RunFilter(image, std::vector<int>(1, devices[0]), triangles);
    const bool same = SameMesh(split.mesh, one.mesh);
    std::cout << "{\"n\": " << n << ", \"devices\": \"" << argv[2] << "\", \"slabs\": " << split.slabs << ", \"points\": "
              << split.mesh->GetNumberOfPoints() << ", \"cells\": " << split.mesh->GetNumberOfCells()
              << ", \"update_s\": " << split.update << ", \"upload_extract_s\": " << split.extract << ", \"download_s\": "
              << split.download << ", \"mesh_fill_s\": " << split.fill << ", \"device_s\": " << split.device
              << ", \"single\": {\"update_s\": " << one.update << ", \"upload_extract_s\": " << one.extract
              << ", \"download_s\": " << one.download << ", \"mesh_fill_s\": " << one.fill << ", \"device_s\": " << one.device
              << "}, \"same_bytes\": " << (same ? "true" : "false") << "}" << std::endl;
    return same ? 0 : 1;
    }
  catch (itk::ExceptionObject &e)
    {
    std::cerr << e << std::endl;
    return 1;
    }
}
