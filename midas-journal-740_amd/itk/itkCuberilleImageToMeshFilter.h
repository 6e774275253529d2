// itkCuberilleImageToMeshFilter.h -- MI355X drop-in for the filter of midas-journal-740.
//
// Same class name, namespace, template parameters (and default), base class and public surface
// as /root/reference/Source/itkCuberilleImageToMeshFilter.h:110-236, so that the reference's
// Testing/CuberilleTest01.cxx and Source/examples.cxx compile against it unchanged.  Nothing of
// the reference's CPU algorithm lives here: GenerateData() (implementation file) marshals the
// image and the eight parameters into the C ABI of include/cuberille_hip.h, the HIP kernels in
// libcuberille_hip.so do the work on the GPU, and the flat buffers that come back are poured into
// the itk::Mesh with ITK's own ownership rules.  Builds against real ITK 3.x/4.x headers, or
// against the ITK-lite headers in itk_lite/ when ITK is not installed.
#ifndef __itkCuberilleImageToMeshFilter_h
#define __itkCuberilleImageToMeshFilter_h

// The reference fixes both at 0 (h:22-23), compiling the two alternative branches of ProjectVertexToIsoSurface out
// (txx:340-437).  A build of the reference with one of them switched on is matched by defining the same macro
// before this header is included: the choice travels as cuberille_params::projection_variant.
#ifndef USE_ADVANCED_PROJECTION
#define USE_ADVANCED_PROJECTION 0
#endif
#ifndef USE_LINESEARCH_PROJECTION
#define USE_LINESEARCH_PROJECTION 0
#endif
// ... and h:21 fixes this one at 0 (itk::GradientImageFilter); 1: itk::GradientRecursiveGaussianImageFilter with
// sigma = the largest spacing (txx:488-491), as cuberille_params::gradient_variant -- ITK's filter restated, parity unpinned
#ifndef USE_GRADIENT_RECURSIVE_GAUSSIAN
#define USE_GRADIENT_RECURSIVE_GAUSSIAN 0
#endif

#include "itkMacro.h"
#include "itkMesh.h"
#include "itkImageToMeshFilter.h"
#include "itkCellInterface.h"
#include "itkTriangleCell.h"
#include "itkQuadrilateralCell.h"
#include "itkDefaultStaticMeshTraits.h"
#include "itkConstShapedNeighborhoodIterator.h"
#include "itkLinearInterpolateImageFunction.h"
#include "itkGradientImageFilter.h"
#include "itkVectorLinearInterpolateImageFunction.h"
#include "itkNumericTraits.h"

#include <string>
#include <vector>

#include "cuberille_hip.h"

namespace itk
{

namespace cuberille_detail
{
// process-wide: do the filters constructed from now on set up their GPU context in the constructor (see SetEagerDeviceSetup)
inline bool &EagerDeviceSetup() { static bool on = true; return on; }
// (itkCuberilleImageToMeshFilter.txx) an image as the C ABI takes it; false when nothing is buffered
template <class TImage> bool DescribeImage(const TImage *image, ::cuberille_image_desc &desc);
}


template <class TInputImage, class TOutputMesh,
          class TInterpolator = itk::LinearInterpolateImageFunction<TInputImage> >
class ITK_EXPORT CuberilleImageToMeshFilter : public ImageToMeshFilter<TInputImage, TOutputMesh>
{
public:
  typedef CuberilleImageToMeshFilter Self;
  typedef ImageToMeshFilter<TInputImage, TOutputMesh> Superclass;
  typedef SmartPointer<Self> Pointer;
  typedef SmartPointer<const Self> ConstPointer;

  itkNewMacro(Self);
  itkTypeMacro(CuberilleImageToMeshFilter, ImageToMeshFilter);

  // -- output side (reference h:127-145) --
  typedef TOutputMesh OutputMeshType;
  typedef typename OutputMeshType::Pointer OutputMeshPointer;
  typedef typename OutputMeshType::MeshTraits OutputMeshTraits;
  typedef typename OutputMeshType::PointType OutputPointType;
  typedef typename OutputMeshType::PointType PointType;
  typedef typename OutputMeshTraits::PixelType OutputPixelType;
  typedef typename OutputMeshType::CellTraits CellTraits;
  typedef typename OutputMeshType::PointsContainer PointsContainer;
  typedef typename OutputMeshType::PointsContainerPointer PointsContainerPointer;
  typedef typename OutputMeshType::CellsContainer CellsContainer;
  typedef typename OutputMeshType::CellsContainerPointer CellsContainerPointer;
  typedef typename OutputMeshType::PointIdentifier PointIdentifier;
  typedef typename OutputMeshType::CellIdentifier CellIdentifier;
  typedef CellInterface<OutputPixelType, CellTraits> CellInterfaceType;
  typedef TriangleCell<CellInterfaceType> TriangleCellType;
  typedef typename TriangleCellType::SelfAutoPointer TriangleAutoPointer;
  typedef typename TriangleCellType::CellAutoPointer TriangleCellAutoPointer;
  typedef QuadrilateralCell<CellInterfaceType> QuadrilateralCellType;
  typedef typename QuadrilateralCellType::SelfAutoPointer QuadrilateralAutoPointer;
  typedef typename QuadrilateralCellType::CellAutoPointer QuadrilateralCellAutoPointer;

  // -- input side (reference h:147-159) --
  typedef TInputImage InputImageType;
  typedef typename InputImageType::Pointer InputImagePointer;
  typedef typename InputImageType::ConstPointer InputImageConstPointer;
  typedef typename InputImageType::PixelType InputPixelType;
  typedef typename InputImageType::SizeType SizeType;
  typedef typename InputImageType::SpacingType SpacingType;
  typedef typename InputImageType::SpacingValueType SpacingValueType;
  typedef typename InputImageType::IndexType IndexType;
  typedef TInterpolator InterpolatorType;
  typedef typename InterpolatorType::Pointer InterpolatorPointer;
  typedef typename InterpolatorType::OutputType InterpolatorOutputType;

  // -- names the reference exposes for its CPU internals (h:162-173); kept so user code that
  //    mentions them still compiles, unused by the GPU path --
  typedef ConstShapedNeighborhoodIterator<InputImageType> InputImageIteratorType;
  typedef GradientImageFilter<InputImageType> GradientFilterType;
  typedef typename GradientFilterType::Pointer GradientFilterPointer;
  typedef typename GradientFilterType::OutputImageType GradientImageType;
  typedef typename GradientImageType::Pointer GradientImagePointer;
  typedef typename GradientFilterType::OutputPixelType GradientPixelType;
  typedef itk::VectorLinearInterpolateImageFunction<GradientImageType> GradientInterpolatorType;
  typedef typename GradientInterpolatorType::Pointer GradientInterpolatorPointer;

  /** Iso-surface value: pixels >= this value are inside (reference h:180-181, txx:139-141). */
  itkGetMacro(IsoSurfaceValue, InputPixelType);
  itkSetMacro(IsoSurfaceValue, InputPixelType);

  /** The image to polygonize (reference h:184, txx:53-56). */
  virtual void SetInput(const InputImageType *inputImage);

  /** Interpolator (reference h:187-188).  The kernels implement LinearInterpolateImageFunction<TInputImage,double> and,
   *  through SetBSplineOnDevice below, BSplineInterpolateImageFunction<TInputImage,float,float> / <...,double,double> of
   *  spline order 3 (the reference driver's USE_BSPLINE_INTERPOLATOR configuration, Testing/CuberilleTest01.cxx:148-151);
   *  with any other type the GPU still does the topology and the lattice points, and the walk of txx:439-474 runs on
   *  the host through the user's Evaluate() -- on the calling thread, as the reference does (txx:455), unless
   *  SetHostWalkThreads asks for more (the interpolator must then be safe to call from several threads at once). */
  itkGetObjectMacro(Interpolator, InterpolatorType);
  itkSetObjectMacro(Interpolator, InterpolatorType);

  /** Triangles (true, default) or quadrilaterals (reference h:193-195). */
  itkGetMacro(GenerateTriangleFaces, bool);
  itkSetMacro(GenerateTriangleFaces, bool);
  itkBooleanMacro(GenerateTriangleFaces);

  /** Project vertices onto the iso-surface (default true; reference h:199-201). */
  itkGetMacro(ProjectVerticesToIsoSurface, bool);
  itkSetMacro(ProjectVerticesToIsoSurface, bool);
  itkBooleanMacro(ProjectVerticesToIsoSurface);

  /** Projection knobs with the reference's clamps (h:209-228); defaults 0.5, max spacing / 4, 0.95, 50. */
  itkGetMacro(ProjectVertexSurfaceDistanceThreshold, double);
  itkSetClampMacro(ProjectVertexSurfaceDistanceThreshold, double, 0.0, NumericTraits<InputPixelType>::max());
  itkGetMacro(ProjectVertexStepLength, double);
  itkSetClampMacro(ProjectVertexStepLength, double, 0.0, 100000.0);
  itkGetMacro(ProjectVertexStepLengthRelaxationFactor, double);
  itkSetClampMacro(ProjectVertexStepLengthRelaxationFactor, double, 0.0, 1.0);
  itkGetMacro(ProjectVertexMaximumNumberOfSteps, unsigned int);
  itkSetMacro(ProjectVertexMaximumNumberOfSteps, unsigned int);

  /** Not in the reference: GPU device to run on (default 0), and the device time in seconds of
   *  the last GenerateData() (all kernels, excluding the PCIe copies and the itk::Mesh fill). */
  itkGetMacro(Device, int);
  itkSetMacro(Device, int);
  itkGetMacro(LastDeviceSeconds, double);
  /** Not in the reference: seconds the last GenerateData() spent pouring the flat buffers into the output
   *  mesh (all cells in one slab the mesh carries in its MetaDataDictionary, CellsAllocatedAsStaticArray, where the
   *  reference's txx:310-329 makes one heap object per face), and a way around that cost for callers that only want the file: the mesh of the last Update(), written as the legacy-ASCII VTK
   *  polydata itk::VTKPolyDataWriter would give for GetOutput(), straight from the device buffers. */
  itkGetMacro(LastMeshFillSeconds, double);
  /** Wall time of the last update's cuberille_extract_host call (upload overlapped with the sweep, then the rest
   * of the extraction) and of copying the flat mesh buffers back to the host. */
  itkGetMacro(LastExtractSeconds, double);
  itkGetMacro(LastDownloadSeconds, double);
  void WriteLastMeshAsVTKPolyData(const char *fileName, int threads = 0);
  /** Not in the reference: seconds the device of this filter takes to receive `bytes` from pinned host memory
   *  (cuberille_debug_h2d_seconds) -- what the upload inside Update() is measured against. */
  double MeasureHostToDeviceSeconds(unsigned long long bytes);
  /** Not in the reference: host threads of the walk taken for a TInterpolator the kernels do not implement.
   *  Default 1 -- the reference calls Evaluate() from one thread (txx:455) and an interpolator may keep mutable
   *  state; more only for interpolators whose Evaluate() const is thread-safe. */
  itkGetMacro(HostWalkThreads, unsigned int);
  itkSetClampMacro(HostWalkThreads, unsigned int, 1u, 256u);
  /** Not in the reference.  By default the constructor sets up the GPU context (runtime start, code objects, a toy
   *  extraction: 100-300 ms once per process) and SetInput sizes the device workspace for its image, so that the ONE cold
   *  Update() the reference's driver times (Testing/CuberilleTest01.cxx:158-160) is the extraction alone; the cost has not
   *  gone away -- profiles/r4_cold_update.log reports constructor and SetInput beside Update().  A process that builds
   *  filters it may never update, forks after constructing them, or picks the device later (SetDevice) turns that off for
   *  the filters it constructs afterwards: everything then happens inside the first Update(), as in round 3. */
  static void SetEagerDeviceSetup(bool on) { cuberille_detail::EagerDeviceSetup() = on; }
  static bool GetEagerDeviceSetup() { return cuberille_detail::EagerDeviceSetup(); }
  /** Not in the reference.  The context keeps the flat mesh in host memory of its own between updates (the second mesh of
   *  a process then copies at the link's rate); true gives that memory -- about 1.125 times the flat mesh -- back to the
   *  system as soon as the itk::Mesh is filled (default false). */
  itkGetMacro(ReleaseHostMeshAfterFill, bool);
  itkSetMacro(ReleaseHostMeshAfterFill, bool);
  itkBooleanMacro(ReleaseHostMeshAfterFill);

  /** Not in the reference -- its behaviour, on request.  The reference builds its gradient image and gradient interpolator
   *  only while the interpolator is null (txx:484) and never resets it: from the second Update() of a filter object on, the
   *  walk follows the gradient of the image the FIRST projecting Update() saw, whatever the input is by then.  This drop-in
   *  uses the current input's gradient; true makes the filter object behave like the reference's, update for update
   *  (cuberille_hold_gradient: the first input's gradient image stays on the device, 12 bytes per voxel).  Default false.
   *  Takes effect with the default LinearInterpolateImageFunction (the device walk); setting it back to false drops the
   *  held image. */
  itkGetMacro(ReproduceStaleGradient, bool);
  itkSetMacro(ReproduceStaleGradient, bool);
  itkBooleanMacro(ReproduceStaleGradient);

  /** Not in the reference.  With TInterpolator = BSplineInterpolateImageFunction<TInputImage, float, float> or
   *  <TInputImage, double, double> whose spline order is 3 at Update(), projection on, the default projection branch, the
   *  central-difference gradient and ReproduceStaleGradient off, the walk runs on the GPU (cuberille_set_interpolator):
   *  the library computes the coefficient image itself and evaluates the 64 taps there, and the quads are split on the
   *  device.  The user's interpolator object then only supplies its spline order; it is not given the image (that would
   *  cost the host prefilter the device route exists to avoid).  The device route restates itk_lite/itkBSplineLite.h bit
   *  for bit; against real ITK's class it may differ in the last bits.  false: every update
   *  walks on the host through the user's own object -- with real ITK, the way to get ITK's own coefficients.  Default
   *  true.  Every other configuration takes the host walk whatever this says. */
  itkGetMacro(BSplineOnDevice, bool);
  itkSetMacro(BSplineOnDevice, bool);
  itkBooleanMacro(BSplineOnDevice);

  /** Not in the reference -- what its class comment (above) tells the caller to do by hand.  PadBorderOn(): Update() gives the
   *  mesh the filter gives for the output of itk::ConstantPadImageFilter with a pad of one pixel of GetBorderPadValue() on
   *  every side of the input (the region grown by one, its start index one lower, the same origin, spacing and direction):
   *  a surface that meets the image border is closed there -- the same points, bit for bit, and cells as pad-then-filter.
   *  No padded copy of the image is made, on the host or on the device (cuberille_set_border).  BorderPadValue defaults
   *  to NumericTraits<InputPixelType>::Zero like the pad filter's constant; signed CT data wants its minimum instead.
   *  Offered where the device walks (or nothing is projected): with SetDevices of more than one device, the B-spline
   *  interpolator, ReproduceStaleGradient, the compiled-out projection / gradient variants or an interpolator that takes
   *  the host walk (the user's object is bound to the unpadded image) Update() throws with the library's message.
   *  Default off: the reference's behaviour. */
  itkGetMacro(PadBorder, bool);
  itkSetMacro(PadBorder, bool);
  itkBooleanMacro(PadBorder);
  itkGetMacro(BorderPadValue, InputPixelType);
  itkSetMacro(BorderPadValue, InputPixelType);

  /** Not in the reference -- what a caller does there with itk::ExtractImageFilter / RegionOfInterestImageFilter first.
   *  SetExtractionRegion(r): Update() gives the mesh the filter gives for the box r of the input as an image of its own
   *  whose region keeps the index (size r.GetSize(), index r.GetIndex(), the same origin, spacing and direction): the same
   *  points, bit for bit, and cells as crop-then-filter.  r is in ITK index space and must lie inside the input's
   *  GetBufferedRegion(), else Update() throws.  No cropped copy of the image is made, on the host or on the device: only
   *  the box's rows cross the link, straight from the input's buffer (cuberille_set_region).  Offered where the device
   *  walks (or nothing is projected): with SetDevices of more than one device, the B-spline interpolator,
   *  ReproduceStaleGradient, PadBorderOn(), the compiled-out projection / gradient variants or an interpolator that takes
   *  the host walk (the user's object is bound to the whole image) Update() throws.  ClearExtractionRegion(): the default,
   *  the whole buffered region. */
  typedef typename InputImageType::RegionType RegionType;
  void SetExtractionRegion(const RegionType &region) { m_ExtractionRegion = region; m_HasExtractionRegion = true; this->Modified(); }
  void ClearExtractionRegion() { m_HasExtractionRegion = false; this->Modified(); }
  const RegionType &GetExtractionRegion() const { return m_ExtractionRegion; }
  bool HasExtractionRegion() const { return m_HasExtractionRegion; }

  /** Not in the reference -- what a caller does there with itk::BinaryThresholdImageFilter first (the reference's own driver
   *  holds that filter ready, test:80,126-132).  SetInsideBand(lower, upper) + InsideBandOn(): Update() gives the mesh the
   *  filter gives for the output of itk::BinaryThresholdImageFilter<TInputImage, TInputImage> with those thresholds and
   *  the inside / outside values of SetBandValues (defaults NumericTraits<InputPixelType>::One / Zero, not the threshold
   *  filter's max / zero: a label mask) -- (lower <= pixel && pixel <= upper) ? inside : outside, a NaN pixel outside -- the
   *  same points, bit for bit, and cells as threshold-then-filter; the iso value applies to that binary image.  No
   *  thresholded copy of the image is made, on the host or on the device (cuberille_set_band).  lower > upper makes Update()
   *  throw, as the threshold filter does.  Offered where the device walks (or nothing is projected): with SetDevices of
   *  more than one device, the B-spline interpolator, ReproduceStaleGradient, PadBorderOn(), SetExtractionRegion, the
   *  compiled-out projection / gradient variants or an interpolator that takes the host walk (the user's object is bound
   *  to the image, not to the binary one) Update() throws with the library's message.  Default off: the reference's
   *  behaviour. */
  void SetInsideBand(InputPixelType lower, InputPixelType upper)
    {
    if (m_BandLower != lower || m_BandUpper != upper) { m_BandLower = lower; m_BandUpper = upper; this->Modified(); }
    }
  void SetBandValues(InputPixelType inside, InputPixelType outside)
    {
    if (m_BandInside != inside || m_BandOutside != outside) { m_BandInside = inside; m_BandOutside = outside; this->Modified(); }
    }
  itkGetMacro(InsideBand, bool);
  itkSetMacro(InsideBand, bool);
  itkBooleanMacro(InsideBand);
  InputPixelType GetBandLower() const { return m_BandLower; }
  InputPixelType GetBandUpper() const { return m_BandUpper; }
  InputPixelType GetBandInsideValue() const { return m_BandInside; }
  InputPixelType GetBandOutsideValue() const { return m_BandOutside; }

  /** Not in the reference -- the vector its walk evaluates in every pass and throws away (normal =
   *  m_GradientInterpolator->Evaluate(vertex); normal.Normalize(), txx:451-452).  GeneratePointNormalsOn(): Update() also
   *  fills GetPointNormals() with that vector at every point's FINAL position -- 3 floats per point id, contiguous -- computed on
   *  the device by a pass of its own behind the walk (cuberille_set_point_normals): the central-difference gradient of the
   *  input, interpolated linearly at the point and normalised, to the letter of the walk's contract.  It points towards
   *  increasing pixel values -- into an object brighter than its surroundings -- and a zero gradient gives NaN.  It stays an
   *  accessor, not mesh point data: the mesh's pixel type is the caller's scalar.  The mesh itself is unchanged.  Offered where
   *  the device walks (or nothing is projected), PadBorderOn(), SetExtractionRegion and InsideBandOn() included; with an
   *  interpolator that takes the host walk the library never sees the final vertices, and with SetDevices of more than one
   *  device, ReproduceStaleGradient or USE_GRADIENT_RECURSIVE_GAUSSIAN the library refuses: Update() throws an
   *  itk::ExceptionObject that says so.  Default off: the array is empty. */
  itkGetMacro(GeneratePointNormals, bool);
  itkSetMacro(GeneratePointNormals, bool);
  itkBooleanMacro(GeneratePointNormals);
  const std::vector<float> &GetPointNormals() const { return m_PointNormals; }

  /** The switch of this filter's maintained successor; the reference reserves the place with a commented-out
   *  mesh->SetCellData( id, (OutputPixelType)0 ) behind every cell it adds (txx:314, 321, 330).  SavePixelAsCellDataOn():
   *  Update() also fills GetCellPixels() with the pixel of the inside voxel of each cell's quad -- one InputPixelType per cell
   *  id, both triangles of a quad carrying the quad's -- written on the device by a pass of its own behind the cell pass
   *  (cuberille_set_cell_pixels), and the mesh's cell data with static_cast<OutputPixelType>(pixel) per cell id.  With
   *  InsideBandOn() it is the input's RAW pixel (which label), with PadBorderOn() the padded image's, with SetExtractionRegion
   *  the box's.  Offered on every route of a single device, the host walk included (its triangles repeat the quad's value on the
   *  host); with SetDevices of more than one device the library refuses and Update() throws an itk::ExceptionObject that says
   *  so.  Default off: the array is empty and the mesh has no cell-data container (nor has a mesh without cells, the switch on:
   *  itk::Mesh makes the container with the first SetCellData( id, value )). */
  itkGetMacro(SavePixelAsCellData, bool);
  itkSetMacro(SavePixelAsCellData, bool);
  itkBooleanMacro(SavePixelAsCellData);
  const std::vector<InputPixelType> &GetCellPixels() const { return m_CellPixels; }

  /** Not in the reference: what a caller does with the mesh in itk::ConnectedRegionsMeshFilter, on the device.
   *  GenerateComponentsOn(): Update() also labels the connected surfaces of the output mesh (cuberille_set_components) -- two
   *  points are joined when one cell holds both, components are numbered in the order of their smallest point id -- and fills
   *  GetPointComponents() (one label per point id), GetCellComponents() (per cell id: the component of the cell's first point),
   *  GetComponentCellCounts() (cells per component) and GetNumberOfComponents().  The mesh's cell data stays the cell pixels'.
   *  Offered on every route of a single device (after the host walk's split of quads into triangles the cell labels are
   *  repeated and the counts doubled on the host); with SetDevices of more than one device the library refuses and Update()
   *  throws an itk::ExceptionObject that says so.  Default off: the vectors are empty, the number is 0. */
  itkGetMacro(GenerateComponents, bool);
  itkSetMacro(GenerateComponents, bool);
  itkBooleanMacro(GenerateComponents);
  const std::vector<uint32_t> &GetPointComponents() const { return m_PointComponents; }
  const std::vector<uint32_t> &GetCellComponents() const { return m_CellComponents; }
  const std::vector<uint64_t> &GetComponentCellCounts() const { return m_ComponentCellCounts; }
  size_t GetNumberOfComponents() const { return m_ComponentCellCounts.size(); }

  /** Not in the reference: what a caller does with the mesh afterwards -- interpolator->SetInputImage(other);
   *  interpolator->Evaluate(point) in a loop over mesh->GetPoints() -- on the device, where the mesh already is
   *  (cuberille_set_point_scalars).  SetPointScalarImage(other): `other` is any three-dimensional itk::Image of one of the ten
   *  pixel types, with its own buffered region, spacing, origin and direction; Update() then also fills GetPointScalars() with
   *  one double per point id: itk::LinearInterpolateImageFunction<TScalarImage, double>::Evaluate at the point's FINAL position
   *  where that lies inside the image's buffer (index - 0.5 <= continuous index < index + size - 0.5 on every axis), and
   *  SetPointScalarOutsideValue's value (default: a quiet NaN) elsewhere.  The output mesh's point data holds
   *  static_cast<OutputPixelType>(value) per point.  A null pointer turns it off (the default: GetPointScalars() is empty and
   *  the mesh has no point-data container).  The image's pixels are uploaded ONCE per call of SetPointScalarImage, by the next
   *  Update(), and the filter holds a reference to the image until then: a caller who changes its pixels calls
   *  SetPointScalarImage again.  Not offered with SetDevices of more than one device nor with an interpolator that takes the
   *  host walk (the library never sees the final vertices): Update() throws an itk::ExceptionObject that says "point scalars".
   *  Out of scope: nearest-neighbour and B-spline sampling of the second image, vector images, several second images. */
  template <class TScalarImage> void SetPointScalarImage(const TScalarImage *image)
  {
    static_assert(TScalarImage::ImageDimension == 3, "SetPointScalarImage: the second image is three-dimensional, like the input");
    m_PointScalarImage = image;
    m_PointScalarVoxels = image ? static_cast<const void *>(image->GetBufferPointer()) : 0;
    m_HasPointScalarImage = image != 0;
    m_PointScalarDesc = ::cuberille_image_desc();
    if (image) (void)cuberille_detail::DescribeImage(image, m_PointScalarDesc);      // (false: an empty region, which the library refuses by its dims)
    m_PointScalarUploadedTo = 0;
    this->Modified();
  }
  void SetPointScalarOutsideValue(double v) { m_PointScalarOutsideValue = v; m_PointScalarUploadedTo = 0; this->Modified(); }
  double GetPointScalarOutsideValue() const { return m_PointScalarOutsideValue; }
  const std::vector<double> &GetPointScalars() const { return m_PointScalars; }

  /** Not in the reference: what a caller of itk::ConnectedRegionsMeshFilter does behind the filter -- keep the largest surface,
   *  drop the specks -- on the device, before the output mesh is filled (cuberille_keep_components).
   *  KeepLargestComponentOn(): Update() keeps the one connected surface with the most cells (a tie goes to the component with
   *  the smaller first point id) and drops every other.  SetMinimumComponentCells(n), n > 0: Update() drops every surface of
   *  fewer than n cells (with GenerateTriangleFaces a quad is two cells); behind the largest-component selection where both are
   *  set.  Either one turns the components on for that Update() by itself.  The output mesh, its cell data, GetPointNormals(),
   *  GetCellPixels(), Get*Components() and GetNumberOfComponents() all describe the kept mesh, whose points and cells keep their
   *  order and are numbered anew; a bound above every component yields an empty mesh.  Not offered with SetDevices of more than
   *  one device or with an interpolator that takes the host walk.  Default: off, 0. */
  itkGetMacro(KeepLargestComponent, bool);
  itkSetMacro(KeepLargestComponent, bool);
  itkBooleanMacro(KeepLargestComponent);
  itkGetMacro(MinimumComponentCells, unsigned long long);
  itkSetMacro(MinimumComponentCells, unsigned long long);

  /** Not in the reference.  More than one device id -- ids may repeat: several contexts on one GPU -- makes Update() cut
   *  the volume into z-slabs of equal thickness, one per member of a context group (cuberille_group_extract_host): each
   *  slab and its halo go from the input's buffer straight to its own device, and one mesh comes back, the same ids, cell
   *  order and bits as the single context's.  Empty (the default): the single context on GetDevice(), as before.  Update()
   *  takes the single context all the same for what a slab cannot do: the B-spline walk on the device,
   *  ReproduceStaleGradient, the recursive-Gaussian gradient.  The environment variable CUBERILLE_DEVICES (say "0,1,2,3"
   *  or "0,0"), read by the constructor, gives the default, so that an unchanged driver runs split; a malformed value
   *  makes Update() throw.  GetLastNumberOfSlabs(): the slabs the last Update() was cut into (1: the single context). */
  void SetDevices(const std::vector<int> &devices);
  const std::vector<int> &GetDevices() const { return m_Devices; }
  unsigned int GetLastNumberOfSlabs() const { return m_LastNumberOfSlabs; }

  // THE ACCESSORS AFTER A THROWING Update() -- a refused combination of switches, a region outside the buffer, a failure of the
  // library: GetPointNormals(), GetCellPixels(), GetPointComponents(), GetCellComponents() and GetComponentCellCounts() are all
  // empty and GetNumberOfComponents() is 0, whatever the update before left there: nothing of an earlier mesh is handed out
  // beside an output the pipeline has re-initialised.  The filter object stays usable: the next Update() with an accepted
  // combination gives what a fresh object would.

  /** Not in the reference: the image description and the extraction region as a box of the buffer (all zero: none) that
   *  Update() would hand the library for the current input and SetExtractionRegion; false when nothing is buffered.  Needs no GPU. */
  bool DescribeInput(::cuberille_image_desc &desc, int64_t boxStart[3], int64_t boxSize[3]);

protected:
  CuberilleImageToMeshFilter();
  ~CuberilleImageToMeshFilter();
  void PrintSelf(std::ostream &os, Indent indent) const;

  void GenerateData();
  virtual void GenerateOutputInformation() {}   // as the reference (h:236)

private:
  CuberilleImageToMeshFilter(const Self &);   // not implemented
  void operator=(const Self &);               // not implemented

  InputPixelType m_IsoSurfaceValue;
  InterpolatorPointer m_Interpolator;
  SpacingValueType m_MaxSpacing;
  bool m_GenerateTriangleFaces;
  bool m_ProjectVerticesToIsoSurface;
  double m_ProjectVertexSurfaceDistanceThreshold;
  double m_ProjectVertexStepLength;
  double m_ProjectVertexStepLengthRelaxationFactor;
  unsigned int m_ProjectVertexMaximumNumberOfSteps;
  int m_Device;
  unsigned int m_HostWalkThreads;
  bool m_ReleaseHostMeshAfterFill;
  bool m_ReproduceStaleGradient;
  bool m_BSplineOnDevice;
  bool m_PadBorder;
  InputPixelType m_BorderPadValue;
  RegionType m_ExtractionRegion;
  bool m_HasExtractionRegion;
  bool m_GeneratePointNormals;
  std::vector<float> m_PointNormals;          // GetPointNormals(): filled by Update() with the switch on, else empty
  bool m_SavePixelAsCellData;
  std::vector<InputPixelType> m_CellPixels;   // GetCellPixels(): filled by Update() with the switch on, else empty
  bool m_GenerateComponents;
  bool m_KeepLargestComponent;
  unsigned long long m_MinimumComponentCells;
  std::vector<uint32_t> m_PointComponents, m_CellComponents;   // filled by Update() with the switch on, else empty
  std::vector<uint64_t> m_ComponentCellCounts;
  SmartPointer<const LightObject> m_PointScalarImage;   // SetPointScalarImage: the second image, held until its upload
  const void *m_PointScalarVoxels;
  ::cuberille_image_desc m_PointScalarDesc;
  bool m_HasPointScalarImage;
  double m_PointScalarOutsideValue;
  ::cuberille_ctx *m_PointScalarUploadedTo;   // the context that holds the copy of the image as last set (null: none does)
  std::vector<double> m_PointScalars;         // GetPointScalars(): filled by Update() with a second image set, else empty
  bool m_InsideBand;
  InputPixelType m_BandLower, m_BandUpper, m_BandInside, m_BandOutside;
  void ClearAttributeOutputs();               // the six vectors above, emptied: how every Update() begins and how a throwing one ends
  void BandArguments(double v[4], int64_t vi[4]) const;   // the four members as cuberille_set_band / _band_check take them
  // SetExtractionRegion as a position in the buffer `desc` describes: ITK index - the buffer's start index (all zero: none)
  void BufferBox(const ::cuberille_image_desc &desc, int64_t start[3], int64_t size[3]) const;
  // PadBorder onto ctx and, where asked for, the extraction region (a group's members take none) and the band (SetInput's
  // reservation needs none), each on or off as the members say; returns null, or the name of the setter that refused (its
  // text: cuberille_last_error(ctx))
  const char *ApplyView(::cuberille_ctx *ctx, const ::cuberille_image_desc &desc, bool withBox, bool withBand) const;
  double m_LastDeviceSeconds;
  double m_LastMeshFillSeconds;
  double m_LastExtractSeconds;
  double m_LastDownloadSeconds;
  ::cuberille_ctx    *m_Context;
  int m_ContextDevice;                        // the device m_Context lives on (SetDevice may come after the constructor)
  bool AcquireContext(bool mustSucceed);      // create + cuberille_warm_up when there is none (or it sits on another device)
  std::vector<int> m_Devices;                 // SetDevices / CUBERILLE_DEVICES: more than one = the group route
  std::string m_DevicesError;                 // a malformed CUBERILLE_DEVICES, thrown by Update()
  ::cuberille_group *m_Group;
  std::vector<int> m_GroupDevices;            // the devices m_Group was made for
  bool m_LastUpdateGrouped;                   // the last Update() ran on m_Group: its buffers are the ones to read
  unsigned int m_LastNumberOfSlabs;
  bool AcquireGroup(bool mustSucceed);        // create + cuberille_group_warm_up for m_Devices
};

} // end namespace itk

#ifndef ITK_MANUAL_INSTANTIATION
#include "itkCuberilleImageToMeshFilter.txx"
#endif

#endif
