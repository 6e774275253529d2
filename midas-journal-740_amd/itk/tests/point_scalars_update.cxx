// SetPointScalarImage() of the drop-in against the host loop it replaces: (a) the filter on a `short` input with a `float`
// second image of another size and geometry (spacing, origin, a rotated direction, a start index off zero) --
// GetPointScalars() holds one double per point id, the mesh's point data static_cast<OutputPixelType> of it --, (b) a loop over
// the output mesh's points through itk::LinearInterpolateImageFunction<ScalarImageType, double>::Evaluate where the point
// lies inside the second image's buffer (index - 0.5 <= continuous index < index + size - 0.5 on every axis, the continuous
// index by the library's own arithmetic: the cofactor inverse, the sum in its order) and the outside value elsewhere.  The
// two must be equal bit for bit (a NaN matching a NaN), on the static and on the dynamic mesh traits.  Off again: the
// accessor is empty, the mesh has no point data and the same points.  With an interpolator that takes the host walk, and with
// SetDevices of more than one device, Update() must throw an itk::ExceptionObject that names the point scalars, and the
// accessor is empty afterwards.  Exits non-zero on a difference.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "itkImage.h"
#include "itkMesh.h"
#include "itkDefaultDynamicMeshTraits.h"
#include "itkCuberilleImageToMeshFilter.h"

typedef itk::Image<short, 3> ImageType;
typedef itk::Image<float, 3> ScalarImageType;
typedef itk::Mesh<float, 3> MeshType;
typedef itk::Mesh<double, 3, itk::DefaultDynamicMeshTraits<double, 3, 3, float> > DynamicMeshType;

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

static bool SameBits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

// the continuous index of p in `image`, operation for operation as the library computes it
static void ContinuousIndex(const ScalarImageType *image, const double p[3], double ci[3])
{
  double i2p[9], p2i[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) i2p[r * 3 + c] = image->GetDirection()[r][c] * image->GetSpacing()[c];
  const double c00 = i2p[4] * i2p[8] - i2p[5] * i2p[7], c01 = i2p[5] * i2p[6] - i2p[3] * i2p[8], c02 = i2p[3] * i2p[7] - i2p[4] * i2p[6];
  const double det = i2p[0] * c00 + i2p[1] * c01 + i2p[2] * c02;
  p2i[0] = c00 / det;
  p2i[1] = (i2p[2] * i2p[7] - i2p[1] * i2p[8]) / det;
  p2i[2] = (i2p[1] * i2p[5] - i2p[2] * i2p[4]) / det;
  p2i[3] = c01 / det;
  p2i[4] = (i2p[0] * i2p[8] - i2p[2] * i2p[6]) / det;
  p2i[5] = (i2p[2] * i2p[3] - i2p[0] * i2p[5]) / det;
  p2i[6] = c02 / det;
  p2i[7] = (i2p[1] * i2p[6] - i2p[0] * i2p[7]) / det;
  p2i[8] = (i2p[0] * i2p[4] - i2p[1] * i2p[3]) / det;
  double cv[3];
  for (int k = 0; k < 3; k++) cv[k] = p[k] - image->GetOrigin()[k];
  for (int r = 0; r < 3; r++)
    {
    double sum = 0.0;
    for (int c = 0; c < 3; c++) sum += p2i[r * 3 + c] * cv[c];
    ci[r] = sum;
    }
}

// the host loop: one value per point of `mesh`; *inside counts the points inside the second image
template <class TMesh> static std::vector<double> HostLoop(const TMesh *mesh, const ScalarImageType *other, double outside, size_t *inside)
{
  typedef itk::LinearInterpolateImageFunction<ScalarImageType, double> InterpolatorType;
  InterpolatorType::Pointer interpolator = InterpolatorType::New();
  interpolator->SetInputImage(other);
  const ScalarImageType::RegionType region = other->GetBufferedRegion();
  std::vector<double> out(mesh->GetNumberOfPoints());
  *inside = 0;
  for (unsigned long i = 0; i < mesh->GetNumberOfPoints(); i++)
    {
    typename TMesh::PointType p;
    mesh->GetPoint(i, &p);
    const double pd[3] = {static_cast<double>(p[0]), static_cast<double>(p[1]), static_cast<double>(p[2])};
    double ci[3];
    ContinuousIndex(other, pd, ci);
    bool in = true;
    for (int k = 0; k < 3; k++)
      in = in && static_cast<double>(region.GetIndex()[k]) - 0.5 <= ci[k] &&
           ci[k] < static_cast<double>(region.GetIndex()[k] + static_cast<long>(region.GetSize()[k])) - 0.5;
    InterpolatorType::PointType q;
    for (int k = 0; k < 3; k++) q[k] = pd[k];
    out[i] = in ? interpolator->Evaluate(q) : outside;
    *inside += in ? 1 : 0;
    }
  return out;
}

template <class TMesh> static bool Run(const ImageType *image, const ScalarImageType *other, double outside, const char *what, std::vector<float> *pointsOut)
{
  typedef itk::CuberilleImageToMeshFilter<ImageType, TMesh> FilterType;
  typename FilterType::Pointer f = FilterType::New();
  f->SetInput(image);
  f->SetIsoSurfaceValue(100);
  f->SetPointScalarImage(other);
  f->SetPointScalarOutsideValue(outside);
  f->Update();
  const TMesh *mesh = f->GetOutput();
  const size_t n = mesh->GetNumberOfPoints();
  const std::vector<double> got = f->GetPointScalars();
  size_t inside = 0;
  const std::vector<double> want = HostLoop(mesh, other, outside, &inside);
  bool ok = n > 1000 && got.size() == n && inside > n / 10 && n - inside > n / 10;
  size_t different = 0, data = 0;
  for (size_t i = 0; ok && i < n; i++)
    {
    if (!SameBits(got[i], want[i])) different++;
    typename TMesh::PixelType v;
    if (!mesh->GetPointData(i, &v) || !SameBits(static_cast<double>(v), static_cast<double>(static_cast<typename TMesh::PixelType>(got[i])))) data++;
    }
  std::cout << what << ": " << n << " points, " << inside << " inside the second image, " << different << " differ from the host loop, "
            << data << " point data differ\n";
  ok = ok && different == 0 && data == 0 && mesh->GetPointData() != 0;
  std::vector<float> points(3 * n);
  for (size_t i = 0; i < n; i++)
    {
    typename TMesh::PointType p;
    mesh->GetPoint(i, &p);
    for (int k = 0; k < 3; k++) points[3 * i + k] = p[k];
    }
  // a second Update() with the same image: no new upload, the same values
  f->Modified();
  f->Update();
  ok = ok && f->GetPointScalars().size() == n && std::memcmp(&f->GetPointScalars()[0], &got[0], n * sizeof(double)) == 0;
  // off again: the accessor is empty, the mesh has no point data and the same points
  f->SetPointScalarImage(static_cast<const ScalarImageType *>(0));
  f->Update();
  bool off = f->GetPointScalars().empty() && f->GetOutput()->GetPointData() == 0 && f->GetOutput()->GetNumberOfPoints() == n;
  for (size_t i = 0; off && i < n; i++)
    {
    typename TMesh::PointType p;
    f->GetOutput()->GetPoint(i, &p);
    for (int k = 0; k < 3; k++) off = off && std::memcmp(&points[3 * i + k], &p[k], sizeof(float)) == 0;
    }
  std::cout << what << ", off again: " << (off ? "empty, no point data, the same mesh" : "DIFFERENT") << "\n";
  if (pointsOut) *pointsOut = points;
  return ok && off;
}

int main()
{
  const int nx = 40, ny = 36, nz = 32;
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
    spacing[0] = 0.7; spacing[1] = 0.7; spacing[2] = 1.5;
    image->SetSpacing(spacing);
    for (int z = 0; z < nz; z++)
      for (int y = 0; y < ny; y++)
        for (int x = 0; x < nx; x++)
          {
          const double r = std::sqrt((x - nx * 0.49) * (x - nx * 0.49) + (y - ny * 0.52) * (y - ny * 0.52) + (z - nz * 0.47) * (z - nz * 0.47));
          image->GetBufferPointer()[(static_cast<size_t>(z) * ny + y) * nx + x] =
            static_cast<short>(300.0 - 15.0 * r + 9.0 * std::sin(0.4 * x) * std::cos(0.3 * y + 0.2 * z));
          }
    // the second image: another size, spacing, origin, a rotation about z, another start index; it covers a part of the surface
    const int mx = 21, my = 17, mz = 13;
    ScalarImageType::Pointer other = ScalarImageType::New();
    ScalarImageType::RegionType oregion;
    ScalarImageType::IndexType ostart;
    ScalarImageType::SizeType osize;
    ostart[0] = -2; ostart[1] = 5; ostart[2] = 1;
    osize[0] = mx; osize[1] = my; osize[2] = mz;
    oregion.SetIndex(ostart);
    oregion.SetSize(osize);
    other->SetRegions(oregion);
    other->Allocate();
    ScalarImageType::SpacingType ospacing;
    ospacing[0] = 1.1; ospacing[1] = 0.9; ospacing[2] = 1.7;
    other->SetSpacing(ospacing);
    ScalarImageType::DirectionType direction;
    direction.SetIdentity();
    direction[0][0] = std::cos(0.3); direction[0][1] = -std::sin(0.3);
    direction[1][0] = std::sin(0.3); direction[1][1] = std::cos(0.3);
    other->SetDirection(direction);
    // (index (0, 0, 0) of the second image near the middle of the first one's extent: about (2.8 + 14, -2.1 + 12.6, 16.5 + 24))
    ScalarImageType::PointType origin;
    origin[0] = 12.0; origin[1] = 1.0; origin[2] = 30.0;
    other->SetOrigin(origin);
    unsigned int seed = 12345u;
    for (size_t i = 0; i < static_cast<size_t>(mx) * my * mz; i++)
      {
      seed = seed * 1664525u + 1013904223u;
      other->GetBufferPointer()[i] = static_cast<float>((seed >> 8) & 0xffff) * 0.37f - 9000.0f;
      }

    std::vector<float> points;
    bool all = Run<MeshType>(image, other, -1.5, "static traits", &points);
    all = Run<DynamicMeshType>(image, other, std::numeric_limits<double>::quiet_NaN(), "dynamic traits", 0) && all;

    // the host-walk route: the library never sees the final vertices
    typedef OwnInterpolator<ImageType> InterpolatorType;
    typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType, InterpolatorType> HostFilterType;
    HostFilterType::Pointer h = HostFilterType::New();
    h->SetInput(image);
    h->SetIsoSurfaceValue(100);
    h->SetPointScalarImage(other.GetPointer());
    bool threw = false;
    try { h->Update(); } catch (itk::ExceptionObject &e) { threw = std::string(e.what()).find("point scalars") != std::string::npos; }
    std::cout << "host walk with a second image: " << (threw ? "refused" : "NOT REFUSED") << "\n";
    all = all && threw && h->GetPointScalars().empty() && h->GetPointNormals().empty() && h->GetCellPixels().empty() &&
          h->GetOutput()->GetNumberOfPoints() == 0;
    h->SetPointScalarImage(static_cast<const ScalarImageType *>(0));
    h->Update();
    all = all && h->GetPointScalars().empty() && h->GetOutput()->GetNumberOfPoints() * 3 == points.size();

    // several devices
    typedef itk::CuberilleImageToMeshFilter<ImageType, MeshType> FilterType;
    FilterType::Pointer g = FilterType::New();
    g->SetInput(image);
    g->SetIsoSurfaceValue(100);
    g->SetDevices(std::vector<int>(2, 0));
    g->SetPointScalarImage(other.GetPointer());
    threw = false;
    try { g->Update(); } catch (itk::ExceptionObject &e) { threw = std::string(e.what()).find("point scalars") != std::string::npos; }
    std::cout << "two devices with a second image: " << (threw ? "refused" : "NOT REFUSED") << "\n";
    all = all && threw && g->GetPointScalars().empty() && g->GetPointNormals().empty() && g->GetCellPixels().empty() &&
          g->GetOutput()->GetNumberOfPoints() == 0;
    std::cout << (all ? "identical" : "DIFFERENT") << "\n";
    return all ? 0 : 1;
    }
  catch (itk::ExceptionObject &e)
    {
    std::cerr << e.what() << "\n";
    return 3;
    }
}
