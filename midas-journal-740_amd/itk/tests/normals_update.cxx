// GeneratePointNormalsOn() of the drop-in against the C ABI it stands on: (a) the filter with the switch on -- GetPointNormals()
// holds 3 floats per point id --, (b) cuberille_set_point_normals + cuberille_extract_host + cuberille_normals_download on a
// context of our own with the same image and parameters.  The two arrays must be equal bit for bit (a NaN matching a NaN), and
// the mesh must be the one the filter gives with the switch off, after which the array is empty; with an interpolator that
// takes the host walk Update() must throw an itk::ExceptionObject that names the point normals.  The image is made here: a
// smooth float field, 48 x 40 x 36, anisotropic spacing, a start index off zero.  Exits non-zero on a difference.
//   usage: normals_update [triangles = 1] [project = 1]
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

// any TInterpolator the device does not run: the host walk
template <class TImage> class OwnInterpolator : public itk::LinearInterpolateImageFunction<TImage, double>
{
public:
  typedef OwnInterpolator Self;
  typedef itk::LinearInterpolateImageFunction<TImage, double> Superclass;
  typedef itk::SmartPointer<Self> Pointer;
  itkNewMacro(Self);
protected:
  OwnInterpolator() {}
};

static bool SameBits(const float *a, const float *b, size_t n)
{
  for (size_t i = 0; i < n; i++)
    if (std::memcmp(a + i, b + i, sizeof(float)) != 0 && !(a[i] != a[i] && b[i] != b[i])) return false;
  return true;
}

static std::vector<float> PointsOf(const MeshType *m)
{
  std::vector<float> out(m->GetNumberOfPoints() * 3);
  for (unsigned long i = 0; i < m->GetNumberOfPoints(); i++)
    {
    MeshType::PointType p;
    m->GetPoint(i, &p);
    for (int k = 0; k < 3; k++) out[3 * i + k] = p[k];
    }
  return out;
}

int main(int argc, char **argv)
{
  const bool triangles = argc > 1 ? std::atoi(argv[1]) != 0 : true;
  const bool project = argc > 2 ? std::atoi(argv[2]) != 0 : true;
  const int nx = 48, ny = 40, nz = 36;
  const float iso = 120.5f;
  try
    {
    ImageType::Pointer image = ImageType::New();
    ImageType::RegionType region;
    ImageType::IndexType start;
    ImageType::SizeType size;
    start[0] = 4; start[1] = -3; start[2] = 11;
    size[0] = nx; size[1] = ny; size[2] = nz;
    region.SetIndex(start);
    region.SetSize(size);
    image->SetRegions(region);
    image->Allocate();
    ImageType::SpacingType spacing;
    spacing[0] = 0.7; spacing[1] = 0.7; spacing[2] = 2.5;
    image->SetSpacing(spacing);
    for (int z = 0; z < nz; z++)
      for (int y = 0; y < ny; y++)
        for (int x = 0; x < nx; x++)
          {
          const double r = std::sqrt((x - nx * 0.49) * (x - nx * 0.49) + (y - ny * 0.52) * (y - ny * 0.52) + (z - nz * 0.47) * (z - nz * 0.47));
          image->GetBufferPointer()[(static_cast<size_t>(z) * ny + y) * nx + x] =
            static_cast<float>(300.0 - 12.5 * r + 9.0 * std::sin(0.4 * x) * std::cos(0.3 * y + 0.2 * z));
          }

    // (a) the filter
    typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType> FilterType;
    FilterType::Pointer f = FilterType::New();
    f->SetInput(image);
    f->SetIsoSurfaceValue(iso);
    f->SetGenerateTriangleFaces(triangles);
    f->SetProjectVerticesToIsoSurface(project);
    f->GeneratePointNormalsOn();
    f->Update();
    const std::vector<float> normals = f->GetPointNormals();
    const std::vector<float> points = PointsOf(f->GetOutput());
    const size_t n = f->GetOutput()->GetNumberOfPoints();
    bool all = n > 1000 && normals.size() == 3 * n;
    std::cout << n << " points, " << normals.size() << " normal components\n";

    // (b) the C ABI
    cuberille_image_desc desc;
    std::memset(&desc, 0, sizeof desc);
    desc.pixel_type = CUBERILLE_PIX_F32;
    desc.dims[0] = nx; desc.dims[1] = ny; desc.dims[2] = nz;
    for (int i = 0; i < 3; i++) { desc.spacing[i] = spacing[i]; desc.direction[4 * i] = 1.0; desc.index_start[i] = start[i]; }
    cuberille_params prm;
    std::memset(&prm, 0, sizeof prm);
    prm.iso_value = iso;
    prm.generate_triangles = triangles ? 1 : 0;
    prm.project_vertices = project ? 1 : 0;
    prm.distance_threshold = 0.5;
    prm.step_length = 2.5 * 0.25;
    prm.relaxation = 0.95;
    prm.max_steps = 50;
    prm.emulate_empty_slice_aliasing = 1;
    cuberille_ctx *ctx = 0;
    cuberille_result res;
    if (cuberille_create(&ctx, 0) != CUBERILLE_OK) { std::cerr << "cuberille_create: " << cuberille_last_error(0) << "\n"; return 3; }
    std::vector<float> cn, cp;
    if (cuberille_set_point_normals(ctx, 1) != CUBERILLE_OK ||
        cuberille_extract_host(ctx, &desc, image->GetBufferPointer(), &prm, &res) != CUBERILLE_OK)
      { std::cerr << "C ABI: " << cuberille_last_error(ctx) << "\n"; cuberille_destroy(ctx); return 3; }
    cn.resize(res.n_points * 3 + 1);
    cp.resize(res.n_points * 3 + 1);
    if (cuberille_normals_download(ctx, &cn[0]) != CUBERILLE_OK || cuberille_mesh_download(ctx, &cp[0], 0) != CUBERILLE_OK)
      { std::cerr << "C ABI: " << cuberille_last_error(ctx) << "\n"; cuberille_destroy(ctx); return 3; }
    cuberille_destroy(ctx);
    const bool same = res.n_points == n && SameBits(&cp[0], &points[0], 3 * n) && SameBits(&cn[0], &normals[0], 3 * n);
    size_t finite = 0;
    for (size_t i = 0; i < normals.size(); i++) finite += normals[i] == normals[i] ? 1 : 0;
    std::cout << "GetPointNormals() against cuberille_normals_download: " << (same ? "same" : "DIFFERENT") << ", " << finite
              << " finite components\n";
    all = all && same && finite > normals.size() / 2;

    // the switch off: the array is empty, the mesh the same
    f->GeneratePointNormalsOff();
    f->Update();
    const std::vector<float> again = PointsOf(f->GetOutput());
    const bool off = f->GetPointNormals().empty() && again.size() == points.size() && SameBits(&again[0], &points[0], points.size());
    std::cout << "GeneratePointNormalsOff: " << (off ? "empty, the same mesh" : "DIFFERENT") << "\n";
    all = all && off;

    // the host-walk route: the library never sees the final vertices
    typedef OwnInterpolator<ImageType> InterpolatorType;
    typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType, InterpolatorType> HostFilterType;
    HostFilterType::Pointer h = HostFilterType::New();
    h->SetInput(image);
    h->SetIsoSurfaceValue(iso);
    h->GeneratePointNormalsOn();
    bool threw = false;
    try { h->Update(); } catch (itk::ExceptionObject &e) { threw = std::string(e.what()).find("point normals") != std::string::npos; }
    std::cout << "host walk with the switch on: " << (threw ? "refused" : "NOT REFUSED") << "\n";
    h->GeneratePointNormalsOff();
    h->Update();
    all = all && threw && h->GetPointNormals().empty() && h->GetOutput()->GetNumberOfPoints() == n;
    std::cout << (all ? "identical" : "DIFFERENT") << "\n";
    return all ? 0 : 1;
    }
  catch (itk::ExceptionObject &e)
    {
    std::cerr << e.what() << "\n";
    return 3;
    }
}
