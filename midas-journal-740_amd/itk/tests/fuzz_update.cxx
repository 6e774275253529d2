// The differential campaign through the drop-in filter (tests/fuzz_dropin.py, tests/test_gpu_dropin_campaign.py): ONE long-lived
// filter object per (pixel type, interpolator type, mesh traits), driven through the cases of a script, every result read back
// through ITK's public mesh API and written as bytes.  Nothing is compared here: the references are Python's.
//
//   fuzz_update run <script> <outdir>     every line of the script in order, in this process; per line L the files
//                                         <outdir>/L.meta (text) and <outdir>/L.<row> (bytes) described at Dump() below
//   fuzz_update dry <script>              no GPU: eager setup off, no Update(); applies each line's setters and prints every
//                                         getter, the cuberille_image_desc and the buffer box Update() would hand over
//
// A script line is a list of key=value words; floating-point values travel as C99 hexadecimal (or nan / inf / -inf), pixel values
// of the integer types as decimal integers (64 bits survive), lists with commas.  What a line does not name is switched back to
// its default, so the line alone says what the object holds -- except the step length, whose value `keep` leaves the object's own
// (the sticky default of txx:82-85), and the object itself, which is the one the lines before used unless the line says fresh=1.
//
//   line=L case=N sub=S                              (sub: what the line is of its case -- main, refusal, first, plain)
//   pix=u8|i8|u16|i16|u32|i32|f32|f64|i64|u64  interp=linear|inherit|bspline32|bspline64  traits=static|dynamic
//   fresh=0|1 eager=0|1 release=0|1
//   vol=<raw file> dims=nx,ny,nz spacing=.. origin=.. direction=<9> start=i,j,k
//   iso=<pixel> tri=0|1 project=0|1 thr=<double> step=<double>|keep relax=<double> maxsteps=<n>
//   devices=<n copies of device 0, 0: none> threads=<n>
//   border=<pixel>  region=i,j,k,nx,ny,nz  band=lower,upper,inside,outside bandon=0|1
//   normals=0|1 celldata=0|1 components=0|1 largest=0|1 mincells=<n> stale=0|1 bsplinedev=0|1 updates=<n>
//
// interp=inherit: a user's class that derives from the linear interpolator and inherits its Evaluate() -- the filter cannot know
// that and walks on the host, which must give the device walk's mesh bit for bit.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "itkImage.h"
#include "itkMesh.h"
#include "itkDefaultDynamicMeshTraits.h"
#include "itkBSplineInterpolateImageFunction.h"
#include "itkCuberilleImageToMeshFilter.h"

typedef std::map<std::string, std::string> Line;

static void die(const std::string &what) { std::fprintf(stderr, "fuzz_update: %s\n", what.c_str()); std::exit(3); }

static const std::string &word(const Line &l, const char *key)
{
  Line::const_iterator it = l.find(key);
  if (it == l.end()) die(std::string("the line has no ") + key);
  return it->second;
}
static bool has(const Line &l, const char *key) { return l.count(key) != 0; }
static std::string word(const Line &l, const char *key, const char *otherwise) { return has(l, key) ? word(l, key) : std::string(otherwise); }
static long long integer(const Line &l, const char *key, long long otherwise) { return has(l, key) ? std::strtoll(word(l, key).c_str(), 0, 10) : otherwise; }
static std::vector<std::string> list(const std::string &text)
{
  std::vector<std::string> out;
  std::stringstream ss(text);
  std::string item;
  while (std::getline(ss, item, ',')) out.push_back(item);
  return out;
}
static std::vector<std::string> list(const Line &l, const char *key, size_t n)
{
  std::vector<std::string> v = list(word(l, key));
  if (v.size() != n) die(std::string(key) + " has not the number of values it takes");
  return v;
}
static double real(const std::string &text) { return std::strtod(text.c_str(), 0); }

// a pixel value from its text, and back: the integer types as decimal integers, the floating types as hexadecimal / nan / inf
template <class T> struct PixelText
{
  static T Parse(const std::string &t)
  {
    if (T(-1) < T(0)) return static_cast<T>(std::strtoll(t.c_str(), 0, 10));
    return static_cast<T>(std::strtoull(t.c_str(), 0, 10));
  }
  static std::string Print(T v)
  {
    char b[64];
    if (T(-1) < T(0)) std::snprintf(b, sizeof b, "%lld", static_cast<long long>(v));
    else std::snprintf(b, sizeof b, "%llu", static_cast<unsigned long long>(v));
    return b;
  }
};
static std::string hexreal(double v) { char b[64]; std::snprintf(b, sizeof b, "%a", v); return b; }
template <> struct PixelText<float>  { static float Parse(const std::string &t) { return std::strtof(t.c_str(), 0); } static std::string Print(float v) { return hexreal(v); } };
template <> struct PixelText<double> { static double Parse(const std::string &t) { return std::strtod(t.c_str(), 0); } static std::string Print(double v) { return hexreal(v); } };

// the user's interpolator of the host-walk route: the linear one's Evaluate(), inherited
template <class TImage> class InheritedLinear : public itk::LinearInterpolateImageFunction<TImage, double>
{
public:
  typedef InheritedLinear Self;
  typedef itk::LinearInterpolateImageFunction<TImage, double> Superclass;
  typedef itk::SmartPointer<Self> Pointer;
  itkNewMacro(Self);
protected:
  InheritedLinear() {}
};

static void put(const std::string &path, const void *p, size_t bytes)
{
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f || (bytes && std::fwrite(p, 1, bytes, f) != bytes)) die("cannot write " + path);
  std::fclose(f);
}
template <class T> static void put(const std::string &path, const std::vector<T> &v) { put(path, v.empty() ? 0 : &v[0], sizeof(T) * v.size()); }

template <class TImage> static typename TImage::Pointer load(const Line &l, const char *prefix)
{
  const std::string p(prefix);
  const std::vector<std::string> dims = list(l, (p + "dims").c_str(), 3), spacing = list(l, (p + "spacing").c_str(), 3),
                                 origin = list(l, (p + "origin").c_str(), 3), direction = list(l, (p + "direction").c_str(), 9),
                                 start = list(l, (p + "start").c_str(), 3);
  typename TImage::Pointer image = TImage::New();
  typename TImage::RegionType region;
  typename TImage::IndexType index;
  typename TImage::SizeType size;
  typename TImage::SpacingType sp;
  typename TImage::PointType org;
  typename TImage::DirectionType dir;
  for (int i = 0; i < 3; i++)
    {
    index[i] = std::strtol(start[i].c_str(), 0, 10);
    size[i] = std::strtoul(dims[i].c_str(), 0, 10);
    sp[i] = real(spacing[i]);
    org[i] = real(origin[i]);
    for (int j = 0; j < 3; j++) dir[i][j] = real(direction[3 * i + j]);
    }
  region.SetIndex(index);
  region.SetSize(size);
  image->SetRegions(region);
  image->SetSpacing(sp);
  image->SetOrigin(org);
  image->SetDirection(dir);
  image->Allocate();
  const size_t n = static_cast<size_t>(size[0]) * size[1] * size[2];
  const std::string path = word(l, (p + "vol").c_str());
  if (path != "-")                                        // (dry: the description alone)
    {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(image->GetBufferPointer(), sizeof(typename TImage::PixelType), n, f) != n) die("cannot read " + path);
    std::fclose(f);
    }
  return image;
}

struct RunnerBase
{
  virtual ~RunnerBase() {}
  virtual void Run(const Line &l, const std::string &out, bool dry) = 0;
};

template <class TPixel, class TInterpolator, class TMesh> struct Runner : RunnerBase
{
  typedef itk::Image<TPixel, 3> ImageType;
  typedef itk::CuberilleImageToMeshFilter<ImageType, TMesh, TInterpolator> FilterType;
  typedef PixelText<TPixel> Text;
  typename FilterType::Pointer filter;
  typename ImageType::Pointer image, first;          // (the filter's input must outlive the line: the next line may not replace it)

  // every setter, from the line or back to the constructor's default -- but the step length, which `keep` leaves alone
  void Apply(const Line &l)
  {
    filter->SetIsoSurfaceValue(Text::Parse(word(l, "iso")));
    filter->SetGenerateTriangleFaces(integer(l, "tri", 1) != 0);
    filter->SetProjectVerticesToIsoSurface(integer(l, "project", 1) != 0);
    filter->SetProjectVertexSurfaceDistanceThreshold(real(word(l, "thr", "0x1p-1")));
    if (word(l, "step", "keep") != "keep") filter->SetProjectVertexStepLength(real(word(l, "step")));
    filter->SetProjectVertexStepLengthRelaxationFactor(real(word(l, "relax", "0x1.e666666666666p-1")));
    filter->SetProjectVertexMaximumNumberOfSteps(static_cast<unsigned int>(integer(l, "maxsteps", 50)));
    filter->SetDevices(std::vector<int>(static_cast<size_t>(integer(l, "devices", 0)), 0));
    filter->SetHostWalkThreads(static_cast<unsigned int>(integer(l, "threads", 1)));
    filter->SetReleaseHostMeshAfterFill(integer(l, "release", 0) != 0);
    filter->SetReproduceStaleGradient(integer(l, "stale", 0) != 0);
    filter->SetBSplineOnDevice(integer(l, "bsplinedev", 1) != 0);
    filter->SetPadBorder(has(l, "border"));
    // (itkSetMacro assigns only where the member != the argument, in ITK as here: -0.0 would not replace the 0.0 a line before
    //  left.  One first: no pad value of a script equals both.)
    filter->SetBorderPadValue(itk::NumericTraits<TPixel>::One);
    filter->SetBorderPadValue(has(l, "border") ? Text::Parse(word(l, "border")) : itk::NumericTraits<TPixel>::Zero);
    if (has(l, "region"))
      {
      const std::vector<std::string> r = list(l, "region", 6);
      typename ImageType::RegionType region;
      typename ImageType::IndexType index;
      typename ImageType::SizeType size;
      for (int i = 0; i < 3; i++) { index[i] = std::strtol(r[i].c_str(), 0, 10); size[i] = std::strtoul(r[3 + i].c_str(), 0, 10); }
      region.SetIndex(index);
      region.SetSize(size);
      filter->SetExtractionRegion(region);
      }
    else filter->ClearExtractionRegion();
    if (has(l, "band"))
      {
      const std::vector<std::string> b = list(l, "band", 4);
      filter->SetInsideBand(Text::Parse(b[0]), Text::Parse(b[1]));
      filter->SetBandValues(Text::Parse(b[2]), Text::Parse(b[3]));
      }
    else
      {
      filter->SetInsideBand(itk::NumericTraits<TPixel>::Zero, itk::NumericTraits<TPixel>::Zero);
      filter->SetBandValues(itk::NumericTraits<TPixel>::One, itk::NumericTraits<TPixel>::Zero);
      }
    filter->SetInsideBand(integer(l, "bandon", 0) != 0);
    filter->SetGeneratePointNormals(integer(l, "normals", 0) != 0);
    filter->SetSavePixelAsCellData(integer(l, "celldata", 0) != 0);
    filter->SetGenerateComponents(integer(l, "components", 0) != 0);
    filter->SetKeepLargestComponent(integer(l, "largest", 0) != 0);
    filter->SetMinimumComponentCells(std::strtoull(word(l, "mincells", "0").c_str(), 0, 10));
  }

  void PrintGetters(const Line &l)
  {
    std::ostringstream o;
    o << "line=" << word(l, "line") << " iso=" << Text::Print(filter->GetIsoSurfaceValue()) << " tri=" << filter->GetGenerateTriangleFaces()
      << " project=" << filter->GetProjectVerticesToIsoSurface() << " thr=" << hexreal(filter->GetProjectVertexSurfaceDistanceThreshold())
      << " step=" << hexreal(filter->GetProjectVertexStepLength()) << " relax=" << hexreal(filter->GetProjectVertexStepLengthRelaxationFactor())
      << " maxsteps=" << filter->GetProjectVertexMaximumNumberOfSteps() << " devices=" << filter->GetDevices().size();
    for (size_t i = 0; i < filter->GetDevices().size(); i++) if (filter->GetDevices()[i] != 0) o << " device_not_0=1";
    o << " threads=" << filter->GetHostWalkThreads() << " release=" << filter->GetReleaseHostMeshAfterFill()
      << " stale=" << filter->GetReproduceStaleGradient() << " bsplinedev=" << filter->GetBSplineOnDevice()
      << " eager=" << FilterType::GetEagerDeviceSetup() << " padborder=" << filter->GetPadBorder()
      << " border=" << Text::Print(filter->GetBorderPadValue()) << " hasregion=" << filter->HasExtractionRegion();
    if (filter->HasExtractionRegion())
      {
      o << " region=";
      for (int i = 0; i < 3; i++) o << filter->GetExtractionRegion().GetIndex()[i] << ",";
      for (int i = 0; i < 3; i++) o << filter->GetExtractionRegion().GetSize()[i] << (i < 2 ? "," : "");
      }
    o << " bandon=" << filter->GetInsideBand() << " band=" << Text::Print(filter->GetBandLower()) << "," << Text::Print(filter->GetBandUpper())
      << "," << Text::Print(filter->GetBandInsideValue()) << "," << Text::Print(filter->GetBandOutsideValue())
      << " normals=" << filter->GetGeneratePointNormals() << " celldata=" << filter->GetSavePixelAsCellData()
      << " components=" << filter->GetGenerateComponents() << " largest=" << filter->GetKeepLargestComponent()
      << " mincells=" << filter->GetMinimumComponentCells();
    cuberille_image_desc desc;
    int64_t boxStart[3], boxSize[3];
    const bool any = filter->DescribeInput(desc, boxStart, boxSize);
    o << " described=" << any << " pixel_type=" << desc.pixel_type << " desc_dims=" << desc.dims[0] << "," << desc.dims[1] << "," << desc.dims[2]
      << " desc_start=" << desc.index_start[0] << "," << desc.index_start[1] << "," << desc.index_start[2];
    o << " desc_spacing=" << hexreal(desc.spacing[0]) << "," << hexreal(desc.spacing[1]) << "," << hexreal(desc.spacing[2]);
    o << " desc_origin=" << hexreal(desc.origin[0]) << "," << hexreal(desc.origin[1]) << "," << hexreal(desc.origin[2]);
    o << " desc_direction=";
    for (int i = 0; i < 9; i++) o << hexreal(desc.direction[i]) << (i < 8 ? "," : "");
    o << " box=" << boxStart[0] << "," << boxStart[1] << "," << boxStart[2] << "," << boxSize[0] << "," << boxSize[1] << "," << boxSize[2];
    std::cout << o.str() << std::endl;
  }

  // What a line leaves in <out>/L.*, all of it through the public API of the mesh and the filter:
  //   meta        threw=0|1, what=<the exception's text, to the end of the line> (a line of its own), points, cells, celldata=0|1 (has
  //               the mesh a cell-data container), celldata_missing (cells GetCellData() has no value for), K, slabs, step
  //   points      mesh->GetPoint(i): 3 coordinates per point, the mesh's coordinate type (float) as bytes
  //   arity       one byte per cell: GetNumberOfPoints() of GetCell(c)
  //   cells       PointIdsBegin() .. of every cell, 8 bytes per id
  //   celldata    GetCellData(c) per cell, the mesh's pixel type as bytes
  //   normals, pixels, pcomp, ccomp, counts   GetPointNormals(), GetCellPixels(), GetPointComponents(), GetCellComponents(),
  //               GetComponentCellCounts() as bytes
  void Dump(const Line &l, const std::string &out, bool threw, const std::string &what)
  {
    const std::string base = out + "/" + word(l, "line") + ".";
    TMesh *mesh = filter->GetOutput();
    const unsigned long nPoints = mesh->GetNumberOfPoints(), nCells = mesh->GetNumberOfCells();
    std::vector<typename TMesh::CoordRepType> pts(3 * static_cast<size_t>(nPoints));
    for (unsigned long i = 0; i < nPoints; i++)
      {
      typename TMesh::PointType p;
      if (!mesh->GetPoint(i, &p)) die("GetPoint has no point " + std::to_string(i));
      for (int k = 0; k < 3; k++) pts[3 * i + k] = p[k];
      }
    std::vector<unsigned char> arity(nCells);
    std::vector<uint64_t> ids;
    std::vector<typename TMesh::CellPixelType> data;
    unsigned long missing = 0;
    for (unsigned long c = 0; c < nCells; c++)
      {
      typename TMesh::CellAutoPointer cell;
      if (!mesh->GetCell(c, cell)) die("GetCell has no cell " + std::to_string(c));
      arity[c] = static_cast<unsigned char>(cell->GetNumberOfPoints());
      for (typename TMesh::CellType::PointIdConstIterator it = cell->PointIdsBegin(); it != cell->PointIdsEnd(); ++it) ids.push_back(*it);
      typename TMesh::CellPixelType v = typename TMesh::CellPixelType();
      if (mesh->GetCellData() && !mesh->GetCellData(c, &v)) missing++;
      if (mesh->GetCellData()) data.push_back(v);
      }
    put(base + "points", pts);
    put(base + "arity", arity);
    put(base + "cells", ids);
    put(base + "celldata", data);
    put(base + "normals", filter->GetPointNormals());
    put(base + "pixels", filter->GetCellPixels());
    put(base + "pcomp", filter->GetPointComponents());
    put(base + "ccomp", filter->GetCellComponents());
    put(base + "counts", filter->GetComponentCellCounts());
    std::ostringstream m;
    std::string flat = what;
    for (size_t i = 0; i < flat.size(); i++) if (flat[i] == '\n') flat[i] = ' ';
    m << "threw=" << threw << "\nwhat=" << flat << "\npoints=" << nPoints << "\ncells=" << nCells << "\ncelldata=" << (mesh->GetCellData() ? 1 : 0)
      << "\ncelldata_missing=" << missing << "\nK=" << filter->GetNumberOfComponents() << "\nslabs=" << filter->GetLastNumberOfSlabs()
      << "\nstep=" << hexreal(filter->GetProjectVertexStepLength()) << "\n";
    const std::string text = m.str();
    put(base + "meta", text.data(), text.size());
  }

  void Run(const Line &l, const std::string &out, bool dry)
  {
    if (filter.IsNull() || integer(l, "fresh", 0) != 0)
      {
      filter = 0;                                      // (the object before goes first: its context with it)
      FilterType::SetEagerDeviceSetup(!dry && integer(l, "eager", 1) != 0);
      filter = FilterType::New();
      }
    image = load<ImageType>(l, "");
    this->Apply(l);
    if (dry)
      {
      filter->SetInput(image);
      this->PrintGetters(l);
      return;
      }
    bool threw = false;
    std::string what;
    try
      {
      if (has(l, "first_vol"))                         // the stale gradient's first image: one projecting Update() of its own
        {
        first = load<ImageType>(l, "first_");
        filter->SetInput(first);
        filter->Update();
        }
      filter->SetInput(image);
      for (long long u = 0; u < integer(l, "updates", 1); u++) filter->Update();
      }
    catch (itk::ExceptionObject &e)
      {
      threw = true;
      what = e.GetDescription();
      }
    this->Dump(l, out, threw, what);
    std::cout << "line " << word(l, "line") << " case " << word(l, "case", "-") << " " << word(l, "sub", "main") << ": "
              << (threw ? "threw" : "ok") << " " << filter->GetOutput()->GetNumberOfPoints() << " points "
              << filter->GetOutput()->GetNumberOfCells() << " cells" << std::endl;
  }
};

template <class TPixel> static RunnerBase *make(const std::string &interp, const std::string &traits)
{
  typedef itk::Image<TPixel, 3> ImageType;
  typedef itk::Mesh<float, 3> StaticMesh;
  typedef itk::Mesh<double, 3, itk::DefaultDynamicMeshTraits<double, 3, 3, float> > DynamicMesh;
  if (interp == "linear" && traits == "static") return new Runner<TPixel, itk::LinearInterpolateImageFunction<ImageType>, StaticMesh>;
  if (interp == "linear" && traits == "dynamic") return new Runner<TPixel, itk::LinearInterpolateImageFunction<ImageType>, DynamicMesh>;
  if (interp == "inherit" && traits == "static") return new Runner<TPixel, InheritedLinear<ImageType>, StaticMesh>;
  if (interp == "bspline32" && traits == "static") return new Runner<TPixel, itk::BSplineInterpolateImageFunction<ImageType, float, float>, StaticMesh>;
  if (interp == "bspline64" && traits == "static") return new Runner<TPixel, itk::BSplineInterpolateImageFunction<ImageType, double, double>, StaticMesh>;
  die("no filter is instantiated for interp=" + interp + " traits=" + traits);
  return 0;
}

static RunnerBase *make(const std::string &pix, const std::string &interp, const std::string &traits)
{
  if (pix == "u8") return make<unsigned char>(interp, traits);
  if (pix == "i8") return make<signed char>(interp, traits);
  if (pix == "u16") return make<unsigned short>(interp, traits);
  if (pix == "i16") return make<short>(interp, traits);
  if (pix == "u32") return make<unsigned int>(interp, traits);
  if (pix == "i32") return make<int>(interp, traits);
  if (pix == "f32") return make<float>(interp, traits);
  if (pix == "f64") return make<double>(interp, traits);
  if (pix == "i64") return make<long long>(interp, traits);
  if (pix == "u64") return make<unsigned long long>(interp, traits);
  die("no pixel type " + pix);
  return 0;
}

int main(int argc, char **argv)
{
  const bool dry = argc == 3 && !std::strcmp(argv[1], "dry"), run = argc == 4 && !std::strcmp(argv[1], "run");
  if (!dry && !run) { std::fprintf(stderr, "usage: fuzz_update run <script> <outdir> | fuzz_update dry <script>\n"); return 1; }
  std::ifstream script(argv[2]);
  if (!script) die(std::string("cannot read ") + argv[2]);
  std::map<std::string, RunnerBase *> objects;          // one per (pixel type, interpolator type, mesh traits), for the whole script
  std::string text;
  int status = 0;
  try
    {
    while (std::getline(script, text))
      {
      if (text.empty() || text[0] == '#') continue;
      Line l;
      std::stringstream ss(text);
      std::string w;
      while (ss >> w)
        {
        const size_t eq = w.find('=');
        if (eq == std::string::npos) die("a word without '=': " + w);
        l[w.substr(0, eq)] = w.substr(eq + 1);
        }
      const std::string key = word(l, "pix") + "/" + word(l, "interp") + "/" + word(l, "traits");
      if (!objects.count(key)) objects[key] = make(word(l, "pix"), word(l, "interp"), word(l, "traits"));
      objects[key]->Run(l, run ? argv[3] : "", dry);
      }
    }
  catch (std::exception &e)
    {
    std::cerr << "fuzz_update: " << e.what() << std::endl;   // (only what is not an itk::ExceptionObject of an Update() arrives here)
    status = 2;
    }
  for (std::map<std::string, RunnerBase *>::iterator it = objects.begin(); it != objects.end(); ++it) delete it->second;
  return status;
}
