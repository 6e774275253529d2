// ITK-lite: itk::BSplineDecompositionImageFilter and itk::BSplineInterpolateImageFunction, restated from ITK 3.x.
//
// This class is the parity target of the library's device B-spline walk (cuberille_set_interpolator): the GPU prefilter
// and the 64-tap value function compute what this header computes, bit for bit, when both are built with
// -ffp-contract=off.  ITK itself is not part of this project, so agreement with ITK's own bytes is UNPINNED, as it is for
// the recursive-Gaussian gradient: every statement below says which ITK 3.x statement it restates, and where this
// restatement departs from ITK it says so (the start index of the buffered region, the physical-to-index matrix,
// coordinates that are not finite).
//
// Evaluate() and EvaluateAtContinuousIndex() touch no mutable member: several threads may call them at once
// (CuberilleImageToMeshFilter::SetHostWalkThreads > 1 is legal with this interpolator).
#ifndef ITK_LITE_BSPLINE_H
#define ITK_LITE_BSPLINE_H

#include "itkLite.h"

#include <cmath>
#include <vector>

namespace itk
{

// ------------------------------------------------------------------------------------------
// BSplineDecompositionImageFilter (ITK 3.x): the interpolation coefficients of a B-spline of order 0-5, mirror boundaries
// ------------------------------------------------------------------------------------------
template <class TInputImage, class TOutputImage> class BSplineDecompositionImageFilter : public Object {
public:
  typedef BSplineDecompositionImageFilter Self;
  typedef SmartPointer<Self> Pointer;
  itkNewMacro(Self);
  itkTypeMacro(BSplineDecompositionImageFilter, ImageToImageFilter);
  typedef TInputImage InputImageType;
  typedef TOutputImage OutputImageType;
  typedef typename TOutputImage::PixelType OutputPixelType;
  typedef double CoeffType;                     // the scratch line is double (ITK: std::vector<CoeffType> m_Scratch)
  static const unsigned int ImageDimension = TInputImage::ImageDimension;

  void SetSplineOrder(unsigned int order)
  {
    if (order > 5) itkExceptionMacro(<< "SplineOrder must be between 0 and 5. Requested spline order has not been implemented yet.");
    m_SplineOrder = order;
    SetPoles();
  }
  unsigned int GetSplineOrder() const { return m_SplineOrder; }
  void SetInput(const TInputImage *image) { m_Input = image; }
  TOutputImage *GetOutput() { return m_Output.GetPointer(); }

  // DataToCoefficientsND: copy first (the input is rounded to the coefficient type), then one axis after the other, every
  // line through the double scratch line and back (rounded to the coefficient type between axes, not inside one)
  void Update()
  {
    if (!m_Input) itkExceptionMacro(<< "no input");
    m_Output = TOutputImage::New();
    m_Output->SetRegions(m_Input->GetBufferedRegion());
    m_Output->SetSpacing(m_Input->GetSpacing());
    m_Output->SetOrigin(m_Input->GetOrigin());
    m_Output->SetDirection(m_Input->GetDirection());
    m_Output->Allocate();
    const size_t nPix = m_Input->GetBufferedRegion().GetNumberOfPixels();
    const typename TInputImage::PixelType *in = m_Input->GetBufferPointer();
    OutputPixelType *out = m_Output->GetBufferPointer();
    for (size_t i = 0; i < nPix; i++) out[i] = static_cast<OutputPixelType>(in[i]);          // CopyImageToImage
    size_t n[ImageDimension], stride[ImageDimension];
    for (unsigned int d = 0, s = 1; d < ImageDimension; d++)
      {
      n[d] = m_Input->GetBufferedRegion().GetSize()[d];
      stride[d] = s;
      s *= static_cast<unsigned int>(n[d]);
      }
    for (unsigned int d = 0; d < ImageDimension; d++)                                         // m_IteratorDirection
      {
      std::vector<CoeffType> scratch(n[d]);
      const size_t lines = n[d] ? nPix / n[d] : 0;
      for (size_t l = 0; l < lines; l++)
        {
        // the first pixel of line l: l counts the lines with the lower axes fastest, axis d left out
        size_t rest = l, base = 0;
        for (unsigned int e = 0; e < ImageDimension; e++)
          {
          if (e == d) continue;
          base += (rest % n[e]) * stride[e];
          rest /= n[e];
          }
        for (size_t j = 0; j < n[d]; j++) scratch[j] = static_cast<CoeffType>(out[base + j * stride[d]]);   // CopyCoefficientsToScratch
        DataToCoefficients1D(scratch);
        for (size_t j = 0; j < n[d]; j++) out[base + j * stride[d]] = static_cast<OutputPixelType>(scratch[j]); // CopyScratchToCoefficients
        }
      }
  }

  // ITK 3.x SetPoles
  void SetPoles()
  {
    switch (m_SplineOrder)
      {
      case 3: m_NumberOfPoles = 1; m_SplinePoles[0] = std::sqrt(3.0) - 2.0; break;
      case 0: m_NumberOfPoles = 0; break;
      case 1: m_NumberOfPoles = 0; break;
      case 2: m_NumberOfPoles = 1; m_SplinePoles[0] = std::sqrt(8.0) - 3.0; break;
      case 4:
        m_NumberOfPoles = 2;
        m_SplinePoles[0] = std::sqrt(664.0 - std::sqrt(438976.0)) + std::sqrt(304.0) - 19.0;
        m_SplinePoles[1] = std::sqrt(664.0 + std::sqrt(438976.0)) - std::sqrt(304.0) - 19.0;
        break;
      case 5:
        m_NumberOfPoles = 2;
        m_SplinePoles[0] = std::sqrt(135.0 / 2.0 - std::sqrt(17745.0 / 4.0)) + std::sqrt(105.0 / 4.0) - 13.0 / 2.0;
        m_SplinePoles[1] = std::sqrt(135.0 / 2.0 + std::sqrt(17745.0 / 4.0)) - std::sqrt(105.0 / 4.0) - 13.0 / 2.0;
        break;
      }
  }

  // ITK 3.x DataToCoefficients1D: gain, then per pole the causal init and recursion, the anti-causal init and recursion
  bool DataToCoefficients1D(std::vector<CoeffType> &c) const
  {
    const size_t N = c.size();
    if (N == 1) return false;                   // required by mirror boundaries: a line of one pixel is left alone
    double c0 = 1.0;
    for (int k = 0; k < m_NumberOfPoles; k++) c0 = c0 * (1.0 - m_SplinePoles[k]) * (1.0 - 1.0 / m_SplinePoles[k]);
    for (size_t n = 0; n < N; n++) c[n] *= c0;
    for (int k = 0; k < m_NumberOfPoles; k++)
      {
      const double z = m_SplinePoles[k];
      SetInitialCausalCoefficient(c, z);
      for (size_t n = 1; n < N; n++) c[n] += z * c[n - 1];
      SetInitialAntiCausalCoefficient(c, z);
      for (long n = static_cast<long>(N) - 2; 0 <= n; n--) c[n] = z * (c[n + 1] - c[n]);
      }
    return true;
  }

  // ITK 3.x SetInitialCausalCoefficient, m_Tolerance = 1e-10: the truncated power sum where the horizon is shorter than
  // the line, else the full mirror sum (z^(N-1) from pow)
  void SetInitialCausalCoefficient(std::vector<CoeffType> &c, double z) const
  {
    const unsigned long N = static_cast<unsigned long>(c.size());
    unsigned long horizon = N;
    double zn = z;
    if (m_Tolerance > 0.0) horizon = static_cast<long>(std::ceil(std::log(m_Tolerance) / std::log(std::fabs(z))));
    if (horizon < N)
      {
      double sum = c[0];
      for (unsigned int n = 1; n < horizon; n++)
        {
        sum += zn * c[n];
        zn *= z;
        }
      c[0] = sum;
      }
    else
      {
      const double iz = 1.0 / z;
      double z2n = std::pow(z, static_cast<double>(N - 1L));
      double sum = c[0] + z2n * c[N - 1L];
      z2n *= z2n * iz;
      for (unsigned int n = 1; n <= N - 2; n++)
        {
        sum += (zn + z2n) * c[n];
        zn *= z;
        z2n *= iz;
        }
      c[0] = sum / (1.0 - zn * zn);
      }
  }

  // ITK 3.x SetInitialAntiCausalCoefficient (mirror boundaries)
  void SetInitialAntiCausalCoefficient(std::vector<CoeffType> &c, double z) const
  {
    const size_t N = c.size();
    c[N - 1] = (z / (z * z - 1.0)) * (z * c[N - 2] + c[N - 1]);
  }

protected:
  BSplineDecompositionImageFilter() : m_SplineOrder(0), m_NumberOfPoles(0), m_Tolerance(1e-10), m_Input(0)
  {
    m_SplinePoles[0] = m_SplinePoles[1] = 0.0;
    SetSplineOrder(3);
  }
  unsigned int m_SplineOrder;
  int m_NumberOfPoles;
  double m_SplinePoles[3];
  double m_Tolerance;
  const TInputImage *m_Input;
  typename TOutputImage::Pointer m_Output;
};

// ------------------------------------------------------------------------------------------
// BSplineInterpolateImageFunction (ITK 3.x), defaults <TImage, double, double> declared in itkLite.h
// ------------------------------------------------------------------------------------------
template <class TImageType, class TCoordRep, class TCoefficientType>
class BSplineInterpolateImageFunction : public Object {
public:
  typedef BSplineInterpolateImageFunction Self;
  typedef SmartPointer<Self> Pointer;
  itkNewMacro(Self);
  itkTypeMacro(BSplineInterpolateImageFunction, InterpolateImageFunction);
  static const unsigned int ImageDimension = TImageType::ImageDimension;
  typedef TImageType InputImageType;
  typedef double OutputType;
  typedef double RealType;
  typedef TCoordRep CoordRepType;
  typedef TCoefficientType CoefficientDataType;
  typedef Image<TCoefficientType, TImageType::ImageDimension> CoefficientImageType;
  typedef BSplineDecompositionImageFilter<TImageType, CoefficientImageType> CoefficientFilter;
  typedef Point<TCoordRep, TImageType::ImageDimension> PointType;
  typedef Point<TCoordRep, TImageType::ImageDimension> ContinuousIndexType;   // (ITK: itk::ContinuousIndex<TCoordRep, N>)
  typedef typename TImageType::IndexType IndexType;

  // orders 0-5; anything else throws (ITK: the decomposition filter's SetSplineOrder)
  void SetSplineOrder(unsigned int order)
  {
    if (order > 5) itkExceptionMacro(<< "SplineOrder must be between 0 and 5. Requested spline order has not been implemented yet.");
    if (order == m_SplineOrder) return;
    m_SplineOrder = order;
    m_CoefficientFilter->SetSplineOrder(order);
    if (m_Image) SetInputImage(m_Image);        // (ITK 3.x recomputes through the pipeline at the next Update; here at once)
    this->Modified();
  }
  unsigned int GetSplineOrder() const { return m_SplineOrder; }

  // computes the coefficient image (ITK 3.x SetInputImage: m_CoefficientFilter->Update())
  void SetInputImage(const TImageType *image)
  {
    m_Image = image;
    if (!image) { m_Coefficients = 0; return; }
    m_CoefficientFilter->SetInput(image);
    m_CoefficientFilter->Update();
    m_Coefficients = m_CoefficientFilter->GetOutput();
    const typename TImageType::RegionType region = image->GetBufferedRegion();
    double i2p[9];
    for (unsigned int r = 0; r < 3; r++)
      {
      m_DataLength[r] = static_cast<long>(region.GetSize()[r]);
      m_Start[r] = static_cast<long>(region.GetIndex()[r]);
      m_Origin[r] = image->GetOrigin()[r];
      for (unsigned int c = 0; c < 3; c++) i2p[r * 3 + c] = image->GetDirection()[r][c] * image->GetSpacing()[c];
      }
    // PhysicalPointToIndex = inverse of Direction * diag(spacing), by cofactors as the library computes it (ITK inverts with
    // vnl's SVD: the matrices may differ in their last bits -- one of the reasons parity with ITK is unpinned)
    const double c00 = i2p[4] * i2p[8] - i2p[5] * i2p[7], c01 = i2p[5] * i2p[6] - i2p[3] * i2p[8];
    const double c02 = i2p[3] * i2p[7] - i2p[4] * i2p[6];
    const double det = i2p[0] * c00 + i2p[1] * c01 + i2p[2] * c02;
    m_P2I[0] = c00 / det; m_P2I[1] = (i2p[2] * i2p[7] - i2p[1] * i2p[8]) / det; m_P2I[2] = (i2p[1] * i2p[5] - i2p[2] * i2p[4]) / det;
    m_P2I[3] = c01 / det; m_P2I[4] = (i2p[0] * i2p[8] - i2p[2] * i2p[6]) / det; m_P2I[5] = (i2p[2] * i2p[3] - i2p[0] * i2p[5]) / det;
    m_P2I[6] = c02 / det; m_P2I[7] = (i2p[1] * i2p[6] - i2p[0] * i2p[7]) / det; m_P2I[8] = (i2p[0] * i2p[4] - i2p[1] * i2p[3]) / det;
  }
  const TImageType *GetInputImage() const { return m_Image; }
  const CoefficientImageType *GetCoefficients() const { return m_Coefficients.GetPointer(); }

  // ImageBase::TransformPhysicalPointToContinuousIndex: point - origin in double, times PhysicalPointToIndex (a double sum
  // from 0 in column order), cast to TCoordRep
  void TransformPointToContinuousIndex(const PointType &point, ContinuousIndexType &index) const
  {
    double cv[3];
    for (unsigned int k = 0; k < 3; k++) cv[k] = static_cast<double>(point[k]) - m_Origin[k];
    for (unsigned int r = 0; r < 3; r++)
      {
      double sum = 0.0;
      for (unsigned int k = 0; k < 3; k++) sum += m_P2I[r * 3 + k] * cv[k];
      index[r] = static_cast<TCoordRep>(sum);
      }
  }

  OutputType Evaluate(const PointType &point) const
  {
    ContinuousIndexType index;
    TransformPointToContinuousIndex(point, index);
    return EvaluateAtContinuousIndex(index);
  }

  OutputType EvaluateAtContinuousIndex(const ContinuousIndexType &x) const
  {
    const unsigned int order = m_SplineOrder;
    long evaluateIndex[3][6];
    double weights[3][6];
    DetermineRegionOfSupport(evaluateIndex, x, order);
    SetInterpolationWeights(x, evaluateIndex, weights, order);
    ApplyMirrorBoundaryConditions(evaluateIndex, order);
    // the (order+1)^3 taps, x fastest (ITK's m_PointsToIndex), one double sum
    const TCoefficientType *coef = m_Coefficients->GetBufferPointer();
    const unsigned int k1 = order + 1;
    const unsigned int nTaps = k1 * k1 * k1;
    double interpolated = 0.0;
    for (unsigned int p = 0; p < nTaps; p++)
      {
      const unsigned int px = p % k1, py = (p / k1) % k1, pz = p / (k1 * k1);
      double w = 1.0;
      w *= weights[0][px];
      w *= weights[1][py];
      w *= weights[2][pz];
      const size_t off = (static_cast<size_t>(evaluateIndex[2][pz]) * static_cast<size_t>(m_DataLength[1]) +
                          static_cast<size_t>(evaluateIndex[1][py])) * static_cast<size_t>(m_DataLength[0]) +
                         static_cast<size_t>(evaluateIndex[0][px]);
      interpolated += w * static_cast<double>(coef[off]);
      }
    return interpolated;
  }

protected:
  BSplineInterpolateImageFunction() : m_SplineOrder(3), m_Image(0)
  {
    m_CoefficientFilter = CoefficientFilter::New();
    m_CoefficientFilter->SetSplineOrder(3);
    for (int i = 0; i < 3; i++) { m_DataLength[i] = 0; m_Start[i] = 0; m_Origin[i] = 0.0; }
    for (int i = 0; i < 9; i++) m_P2I[i] = (i % 4 == 0) ? 1.0 : 0.0;
  }

  // ITK 3.x DetermineRegionOfSupport: odd orders start at floor((float)x) - order/2, even ones at floor((float)(x + 0.5)) -
  // order/2.  ITK 3.x rounds the coordinate to float inside the floor; so does this.  (A coordinate that is not finite, or
  // beyond +-2^40, starts at index 0 instead of ITK's undefined conversion: the weights are NaN or meaningless there
  // anyway, and the taps then stay inside the buffer.)
  static void DetermineRegionOfSupport(long evaluateIndex[3][6], const ContinuousIndexType &x, unsigned int order)
  {
    for (unsigned int n = 0; n < 3; n++)
      {
      double f = (order & 1) ? std::floor(static_cast<float>(x[n])) : std::floor(static_cast<float>(x[n] + 0.5));
      if (!(std::fabs(f) <= 1099511627776.0)) f = 0.0;
      long indx = static_cast<long>(f) - static_cast<long>(order / 2);
      for (unsigned int k = 0; k <= order; k++) evaluateIndex[n][k] = indx++;
      }
  }

  // ITK 3.x SetInterpolationWeights, every case in ITK's own statement order
  static void SetInterpolationWeights(const ContinuousIndexType &x, const long evaluateIndex[3][6], double weights[3][6],
                                      unsigned int order)
  {
    double w, w2, w4, t, t0, t1;
    for (unsigned int n = 0; n < 3; n++)
      {
      switch (order)
        {
        case 3:
          w = x[n] - static_cast<double>(evaluateIndex[n][1]);
          weights[n][3] = (1.0 / 6.0) * w * w * w;
          weights[n][0] = (1.0 / 6.0) + 0.5 * w * (w - 1.0) - weights[n][3];
          weights[n][2] = w + weights[n][0] - 2.0 * weights[n][3];
          weights[n][1] = 1.0 - weights[n][0] - weights[n][2] - weights[n][3];
          break;
        case 0:
          weights[n][0] = 1;
          break;
        case 1:
          w = x[n] - static_cast<double>(evaluateIndex[n][0]);
          weights[n][1] = w;
          weights[n][0] = 1.0 - w;
          break;
        case 2:
          w = x[n] - static_cast<double>(evaluateIndex[n][1]);
          weights[n][1] = 0.75 - w * w;
          weights[n][2] = 0.5 * (w - weights[n][1] + 1.0);
          weights[n][0] = 1.0 - weights[n][1] - weights[n][2];
          break;
        case 4:
          w = x[n] - static_cast<double>(evaluateIndex[n][2]);
          w2 = w * w;
          t = (1.0 / 6.0) * w2;
          weights[n][0] = 1.0 / 2.0 - w;
          weights[n][0] *= weights[n][0];
          weights[n][0] *= (1.0 / 24.0) * weights[n][0];
          t0 = w * (t - 11.0 / 24.0);
          t1 = 19.0 / 96.0 + w2 * (1.0 / 4.0 - t);
          weights[n][1] = t1 + t0;
          weights[n][3] = t1 - t0;
          weights[n][4] = weights[n][0] + t0 + (1.0 / 2.0) * w;
          weights[n][2] = 1.0 - weights[n][0] - weights[n][1] - weights[n][3] - weights[n][4];
          break;
        case 5:
          w = x[n] - static_cast<double>(evaluateIndex[n][2]);
          w2 = w * w;
          weights[n][5] = (1.0 / 120.0) * w * w2 * w2;
          w2 -= w;
          w4 = w2 * w2;
          w -= 1.0 / 2.0;
          t = w2 * (w2 - 3.0);
          weights[n][0] = (1.0 / 24.0) * (1.0 / 5.0 + w2 + w4) - weights[n][5];
          t0 = (1.0 / 24.0) * (w2 * (w2 - 5.0) + 46.0 / 5.0);
          t1 = (-1.0 / 12.0) * w * (t + 4.0);
          weights[n][2] = t0 + t1;
          weights[n][3] = t0 - t1;
          t0 = (1.0 / 16.0) * (9.0 / 5.0 - t);
          t1 = (1.0 / 24.0) * w * (w4 - w2 - 5.0);
          weights[n][1] = t0 + t1;
          weights[n][4] = t0 - t1;
          break;
        }
      }
  }

  // ITK 3.x ApplyMirrorBoundaryConditions (reflection with period 2N-2), taken relative to the buffered region's start
  // index and turned into buffer positions.  ITK 3.x itself ignores the start index (a region that does not start at 0
  // reads outside its buffer there); ITK 4.4 and later reflect once about the first and the last index of the region,
  // which agrees with this for every index less than one line length outside the region.
  void ApplyMirrorBoundaryConditions(long evaluateIndex[3][6], unsigned int order) const
  {
    for (unsigned int n = 0; n < 3; n++)
      {
      const long dataLength2 = 2 * m_DataLength[n] - 2;
      for (unsigned int k = 0; k <= order; k++)
        {
        long e = evaluateIndex[n][k] - m_Start[n];
        if (m_DataLength[n] == 1) e = 0;
        else
          {
          e = (e < 0L) ? (-e - dataLength2 * ((-e) / dataLength2)) : (e - dataLength2 * (e / dataLength2));
          if (m_DataLength[n] <= e) e = dataLength2 - e;
          }
        evaluateIndex[n][k] = e;
        }
      }
  }

  unsigned int m_SplineOrder;
  const TImageType *m_Image;
  typename CoefficientFilter::Pointer m_CoefficientFilter;
  typename CoefficientImageType::Pointer m_Coefficients;
  long m_DataLength[3], m_Start[3];
  double m_Origin[3], m_P2I[9];
};

} // end namespace itk

#endif
