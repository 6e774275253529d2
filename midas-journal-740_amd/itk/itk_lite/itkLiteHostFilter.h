// ITK-lite, host section: the numerical ITK classes that the reference's own filter text (its
// itkCuberilleImageToMeshFilter.h / .txx, compiled UNCHANGED by the test infrastructure's build recipe) calls and that the drop-in
// filter never needs, because its arithmetic runs in the library:
//   ConstShapedNeighborhoodIterator + setConnectivity, GradientImageFilter, LinearInterpolateImageFunction,
//   VectorLinearInterpolateImageFunction.
// Only a translation unit that defines ITK_LITE_HOST_FILTER before its first ITK include sees this file (itkLite.h pulls it
// in at the place of its declaration-only stubs); every other one preprocesses to what it did without it.
//
// Written from ITK 3.x's documented behaviour as the contract I1-I12 of SURVEY.md section 8c states it, in ITK's own
// structure (an operator with coefficients and an inner product, an N-d 2^N neighbour sum).
// Where the contract is silent the choice made here is the one DESIGN.md section 3 lists as unpinned against ITK's bytes.
// It is NOT ITK: it makes the reference's GenerateData() run, so that the filter's own logic -- traversal, lookup maps, ids,
// cell order, split rule, casts and promotions, walk control flow -- is held by compiled reference text.
#ifndef ITK_LITE_HOST_FILTER_H
#define ITK_LITE_HOST_FILTER_H

#ifndef ITK_LITE_H
#error "include itkLite.h (with ITK_LITE_HOST_FILTER defined), not this file"
#endif

namespace itk {

namespace lite {

// (Invert3 and LinearNeighbourhood, which the linear interpolator of itkLite.h shares, are defined there)

// the value of VectorLinearInterpolateImageFunction::Evaluate: components in double; narrows to the pixel's own component
// type where the caller assigns it to one (I7: `normal = m_GradientInterpolator->Evaluate(vertex)`)
template <unsigned int N> class RealVector : public FixedArray<double, N> {
public:
  template <class T> operator CovariantVector<T, N>() const {
    CovariantVector<T, N> v;
    for (unsigned int i = 0; i < N; i++) v[i] = static_cast<T>((*this)[i]);
    return v;
  }
};

}  // namespace lite

// ------------------------------------------------------------------------------------------
// ConstShapedNeighborhoodIterator, radius 1 (I1, I2): walks a region in raster order, first axis fastest; a neighbour
// outside the image's buffered region reads the nearest pixel inside it (ZeroFluxNeumannBoundaryCondition, the default)
// ------------------------------------------------------------------------------------------
template <class TImage> class ConstShapedNeighborhoodIterator {
public:
  typedef TImage ImageType;
  typedef typename TImage::PixelType PixelType;
  typedef typename TImage::IndexType IndexType;
  typedef typename TImage::SizeType SizeType;
  typedef typename TImage::OffsetType OffsetType;
  typedef typename TImage::RegionType RegionType;
  static const unsigned int Dimension = TImage::ImageDimension;

  ConstShapedNeighborhoodIterator(const SizeType &radius, const TImage *image, const RegionType &region)
      : m_Image(image), m_Region(region), m_Radius(radius), m_AtEnd(false) { GoToBegin(); }
  const SizeType &GetRadius() const { return m_Radius; }
  // the active list only says which neighbours an iteration over the shape would visit; GetPixel(offset) reads any
  void ClearActiveList() { m_Active.clear(); }
  void ActivateOffset(const OffsetType &o) { m_Active.push_back(o); }
  void DeactivateOffset(const OffsetType &o) {
    for (size_t i = 0; i < m_Active.size(); i++) {
      bool same = true;
      for (unsigned int k = 0; k < Dimension; k++) same = same && m_Active[i][k] == o[k];
      if (same) { m_Active.erase(m_Active.begin() + i); return; }
    }
  }
  size_t GetActiveIndexListSize() const { return m_Active.size(); }

  void GoToBegin() {
    m_Index = m_Region.GetIndex();
    m_AtEnd = m_Region.GetNumberOfPixels() == 0;
  }
  bool IsAtEnd() const { return m_AtEnd; }
  ConstShapedNeighborhoodIterator &operator++() {
    for (unsigned int k = 0; k < Dimension; k++) {
      if (++m_Index[k] < m_Region.GetIndex()[k] + static_cast<long>(m_Region.GetSize()[k])) return *this;
      m_Index[k] = m_Region.GetIndex()[k];
    }
    m_AtEnd = true;
    return *this;
  }
  IndexType GetIndex() const { return m_Index; }
  PixelType GetCenterPixel() const { return m_Image->GetPixel(m_Index); }
  PixelType GetPixel(const OffsetType &o) const {
    const RegionType &buffered = m_Image->GetBufferedRegion();
    IndexType at;
    for (unsigned int k = 0; k < Dimension; k++) {
      const long lo = buffered.GetIndex()[k], hi = lo + static_cast<long>(buffered.GetSize()[k]) - 1;
      const long v = m_Index[k] + o[k];
      at[k] = v < lo ? lo : (v > hi ? hi : v);
    }
    return m_Image->GetPixel(at);
  }

private:
  const TImage *m_Image;
  RegionType m_Region;
  SizeType m_Radius;
  IndexType m_Index;
  bool m_AtEnd;
  std::vector<OffsetType> m_Active;
};

// itkConnectedComponentAlgorithm.h: activates the face neighbours (2N) or, fully connected, all 3^N - 1
template <class TIterator> TIterator *setConnectivity(TIterator *it, bool fullyConnected = false) {
  typename TIterator::OffsetType offset;
  it->ClearActiveList();
  if (!fullyConnected) {
    for (unsigned int d = 0; d < TIterator::Dimension; d++) {
      for (unsigned int k = 0; k < TIterator::Dimension; k++) offset[k] = 0;
      offset[d] = -1; it->ActivateOffset(offset);
      offset[d] = +1; it->ActivateOffset(offset);
    }
  } else {
    unsigned int total = 1;
    for (unsigned int d = 0; d < TIterator::Dimension; d++) total *= 3;
    for (unsigned int n = 0; n < total; n++) {
      if (n == total / 2) continue;
      unsigned int rest = n;
      for (unsigned int k = 0; k < TIterator::Dimension; k++) { offset[k] = static_cast<long>(rest % 3) - 1; rest /= 3; }
      it->ActivateOffset(offset);
    }
  }
  return it;
}

// ------------------------------------------------------------------------------------------
// GradientImageFilter (I6): per axis a first-derivative operator of radius 1, coefficients (-0.5, 0, +0.5) in
// TOperatorValueType scaled by 1 / spacing (UseImageSpacing, on by default), applied as an inner product accumulated in
// TOperatorValueType over the neighbours in the order (-1, 0, +1), zero-flux border; the vector then goes through the
// direction matrix (UseImageDirection, on by default).  The whole buffered region, on the calling thread.
// ------------------------------------------------------------------------------------------
template <class TImage, class TOperatorValue = float, class TOutputValue = float> class GradientImageFilter : public ProcessObject {
public:
  typedef GradientImageFilter Self;
  typedef SmartPointer<Self> Pointer;
  itkNewMacro(Self);
  itkTypeMacro(GradientImageFilter, ImageToImageFilter);
  static const unsigned int ImageDimension = TImage::ImageDimension;
  typedef TImage InputImageType;
  typedef TOperatorValue OperatorValueType;
  typedef CovariantVector<TOutputValue, TImage::ImageDimension> OutputPixelType;
  typedef Image<OutputPixelType, TImage::ImageDimension> OutputImageType;

  void SetInput(const TImage *image) { this->SetNthInput(0, const_cast<TImage *>(image)); }
  OutputImageType *GetOutput() { return static_cast<OutputImageType *>(this->m_Output.GetPointer()); }
  void SetUseImageSpacing(bool f) { m_UseImageSpacing = f; this->Modified(); }
  void SetUseImageDirection(bool f) { m_UseImageDirection = f; this->Modified(); }

protected:
  GradientImageFilter() : m_UseImageSpacing(true), m_UseImageDirection(true) {
    this->SetNumberOfRequiredInputs(1);
    typename OutputImageType::Pointer o = OutputImageType::New();
    this->SetPrimaryOutput(o.GetPointer());
  }

  virtual void GenerateData() {
    const TImage *in = static_cast<const TImage *>(this->m_Inputs[0].GetPointer());
    OutputImageType *out = this->GetOutput();
    const typename TImage::RegionType &region = in->GetBufferedRegion();
    out->SetRegions(region);
    out->SetSpacing(in->GetSpacing());
    out->SetOrigin(in->GetOrigin());
    out->SetDirection(in->GetDirection());
    out->Allocate();
    // DerivativeOperator of order 1, ScaleCoefficients(1 / spacing)
    OperatorValueType coeff[ImageDimension][3];
    for (unsigned int a = 0; a < ImageDimension; a++) {
      const OperatorValueType base[3] = {static_cast<OperatorValueType>(-0.5), static_cast<OperatorValueType>(0.0), static_cast<OperatorValueType>(0.5)};
      for (int t = 0; t < 3; t++)
        coeff[a][t] = m_UseImageSpacing ? static_cast<OperatorValueType>(base[t] * (1.0 / in->GetSpacing()[a])) : base[t];
    }
    typename TImage::SizeType radius;
    radius.Fill(1);
    ConstShapedNeighborhoodIterator<TImage> it(radius, in, region);
    OutputPixelType *dst = out->GetBufferPointer();
    for (it.GoToBegin(); !it.IsAtEnd(); ++it, ++dst) {
      OperatorValueType local[ImageDimension];
      for (unsigned int a = 0; a < ImageDimension; a++) {
        OperatorValueType sum = 0;
        for (int t = 0; t < 3; t++) {
          typename TImage::OffsetType o;
          for (unsigned int k = 0; k < ImageDimension; k++) o[k] = 0;
          o[a] = t - 1;
          sum += coeff[a][t] * static_cast<OperatorValueType>(it.GetPixel(o));
        }
        local[a] = sum;
      }
      OutputPixelType g;
      if (m_UseImageDirection) {
        // TransformLocalVectorToPhysicalVector: row by column, the running sum kept in the output's component type
        for (unsigned int r = 0; r < ImageDimension; r++) {
          TOutputValue sum = 0;
          for (unsigned int c = 0; c < ImageDimension; c++) sum += in->GetDirection()[r][c] * local[c];
          g[r] = sum;
        }
      } else {
        for (unsigned int r = 0; r < ImageDimension; r++) g[r] = static_cast<TOutputValue>(local[r]);
      }
      *dst = g;
    }
  }

  bool m_UseImageSpacing, m_UseImageDirection;
};

// ------------------------------------------------------------------------------------------
// LinearInterpolateImageFunction (I4, I5): ITK 3.x's N-d form, the 2^N neighbours in counter order (bit k set: the upper
// neighbour along axis k), weights multiplied up along the axes and the sum taken in double; a neighbour of weight zero is
// not read; the loop ends once the weights so far add up to exactly one.  Neighbours clamp into the buffered region.
// ------------------------------------------------------------------------------------------
template <class TInputImage, class TCoordRep = double> class LinearInterpolateImageFunction : public Object {
public:
  typedef LinearInterpolateImageFunction Self;
  typedef SmartPointer<Self> Pointer;
  itkNewMacro(Self);
  itkTypeMacro(LinearInterpolateImageFunction, InterpolateImageFunction);
  static const unsigned int ImageDimension = TInputImage::ImageDimension;
  typedef TInputImage InputImageType;
  typedef double OutputType;
  typedef double RealType;
  typedef Point<TCoordRep, TInputImage::ImageDimension> PointType;
  typedef typename TInputImage::IndexType IndexType;
  void SetInputImage(const TInputImage *image) { m_Image = image; if (image) m_Where.SetImage(image); }
  const TInputImage *GetInputImage() const { return m_Image.GetPointer(); }
  OutputType Evaluate(const PointType &point) const {
    long lower[ImageDimension], upper[ImageDimension];
    double distance[ImageDimension];
    m_Where.Locate(point, lower, upper, distance);
    RealType value = 0.0, totalOverlap = 0.0;
    for (unsigned int counter = 0; counter < (1u << ImageDimension); counter++) {
      double overlap = 1.0;
      IndexType neighbour;
      for (unsigned int k = 0; k < ImageDimension; k++) {
        if (counter & (1u << k)) { neighbour[k] = upper[k]; overlap *= distance[k]; }
        else                     { neighbour[k] = lower[k]; overlap *= 1.0 - distance[k]; }
      }
      if (overlap) {
        value += overlap * static_cast<RealType>(m_Image->GetPixel(neighbour));
        totalOverlap += overlap;
      }
      if (totalOverlap == 1.0) break;
    }
    return value;
  }
protected:
  LinearInterpolateImageFunction() {}
  SmartPointer<const TInputImage> m_Image;
  lite::LinearNeighbourhood<TInputImage> m_Where;
};

// ------------------------------------------------------------------------------------------
// VectorLinearInterpolateImageFunction (I7): the same neighbours and weights, every component summed in double
// ------------------------------------------------------------------------------------------
template <class TInputImage, class TCoordRep = double> class VectorLinearInterpolateImageFunction : public Object {
public:
  typedef VectorLinearInterpolateImageFunction Self;
  typedef SmartPointer<Self> Pointer;
  itkNewMacro(Self);
  itkTypeMacro(VectorLinearInterpolateImageFunction, VectorInterpolateImageFunction);
  static const unsigned int ImageDimension = TInputImage::ImageDimension;
  typedef TInputImage InputImageType;
  typedef typename TInputImage::PixelType PixelType;
  typedef double RealType;
  typedef lite::RealVector<TInputImage::ImageDimension> OutputType;
  typedef Point<TCoordRep, TInputImage::ImageDimension> PointType;
  typedef typename TInputImage::IndexType IndexType;
  void SetInputImage(const TInputImage *image) { m_Image = image; if (image) m_Where.SetImage(image); }
  const TInputImage *GetInputImage() const { return m_Image.GetPointer(); }
  OutputType Evaluate(const PointType &point) const {
    long lower[ImageDimension], upper[ImageDimension];
    double distance[ImageDimension];
    m_Where.Locate(point, lower, upper, distance);
    OutputType output;
    output.Fill(0.0);
    RealType totalOverlap = 0.0;
    for (unsigned int counter = 0; counter < (1u << ImageDimension); counter++) {
      double overlap = 1.0;
      IndexType neighbour;
      for (unsigned int k = 0; k < ImageDimension; k++) {
        if (counter & (1u << k)) { neighbour[k] = upper[k]; overlap *= distance[k]; }
        else                     { neighbour[k] = lower[k]; overlap *= 1.0 - distance[k]; }
      }
      if (overlap) {
        const PixelType &input = m_Image->GetPixel(neighbour);
        for (unsigned int k = 0; k < ImageDimension; k++) output[k] += overlap * static_cast<RealType>(input[k]);
        totalOverlap += overlap;
      }
      if (totalOverlap == 1.0) break;
    }
    return output;
  }
protected:
  VectorLinearInterpolateImageFunction() {}
  SmartPointer<const TInputImage> m_Image;   // keeps the gradient image alive after its filter has gone (txx:493-496)
  lite::LinearNeighbourhood<TInputImage> m_Where;
};

}  // namespace itk

#endif
