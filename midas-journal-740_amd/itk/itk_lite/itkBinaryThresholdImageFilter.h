// ITK-lite: itk::BinaryThresholdImageFilter, RESTATED from ITK's documented behaviour (no ITK source text): the output has
// the input's region, origin, spacing and direction, and every pixel is InsideValue where LowerThreshold <= pixel <=
// UpperThreshold and OutsideValue elsewhere (a NaN pixel fails both comparisons: outside).  Defaults as documented: the
// thresholds span the input pixel type (NonpositiveMin .. max), InsideValue is the output type's max, OutsideValue its Zero.
// Update() throws when LowerThreshold > UpperThreshold.  Host side only; enough of the class for the recipe "threshold, then
// filter" to be written and compared in C++ (tests/band_update.cxx).
#ifndef ITK_LITE_FWD_itkBinaryThresholdImageFilter_H
#define ITK_LITE_FWD_itkBinaryThresholdImageFilter_H
#include "itkLite.h"

#include <limits>

namespace itk {

template <class TInputImage, class TOutputImage> class BinaryThresholdImageFilter : public ProcessObject {
public:
  typedef BinaryThresholdImageFilter Self;
  typedef SmartPointer<Self> Pointer;
  itkNewMacro(Self);
  itkTypeMacro(BinaryThresholdImageFilter, UnaryFunctorImageFilter);
  typedef TInputImage InputImageType;
  typedef TOutputImage OutputImageType;
  typedef typename TInputImage::PixelType InputPixelType;
  typedef typename TOutputImage::PixelType OutputPixelType;

  void SetInput(const TInputImage *image) { this->SetNthInput(0, const_cast<TInputImage *>(image)); }
  TOutputImage *GetOutput() { return static_cast<TOutputImage *>(this->m_Output.GetPointer()); }
  void SetLowerThreshold(InputPixelType v) { m_Lower = v; this->Modified(); }
  void SetUpperThreshold(InputPixelType v) { m_Upper = v; this->Modified(); }
  void SetInsideValue(OutputPixelType v) { m_Inside = v; this->Modified(); }
  void SetOutsideValue(OutputPixelType v) { m_Outside = v; this->Modified(); }
  InputPixelType GetLowerThreshold() const { return m_Lower; }
  InputPixelType GetUpperThreshold() const { return m_Upper; }
  OutputPixelType GetInsideValue() const { return m_Inside; }
  OutputPixelType GetOutsideValue() const { return m_Outside; }

protected:
  BinaryThresholdImageFilter()
      : m_Lower(std::numeric_limits<InputPixelType>::lowest()), m_Upper(std::numeric_limits<InputPixelType>::max()),
        m_Inside(std::numeric_limits<OutputPixelType>::max()), m_Outside(NumericTraits<OutputPixelType>::Zero) {
    this->SetNumberOfRequiredInputs(1);
    typename TOutputImage::Pointer o = TOutputImage::New();
    this->SetPrimaryOutput(o.GetPointer());
  }

  virtual void GenerateData() {
    if (m_Lower > m_Upper) itkExceptionMacro(<< "Lower threshold cannot be greater than upper threshold.");
    const TInputImage *in = static_cast<const TInputImage *>(this->m_Inputs[0].GetPointer());
    TOutputImage *out = this->GetOutput();
    out->SetRegions(in->GetBufferedRegion());
    out->SetSpacing(in->GetSpacing());
    out->SetOrigin(in->GetOrigin());
    out->SetDirection(in->GetDirection());
    out->Allocate();
    const size_t n = in->GetBufferedRegion().GetNumberOfPixels();
    const InputPixelType *src = in->GetBufferPointer();
    OutputPixelType *dst = out->GetBufferPointer();
    for (size_t i = 0; i < n; i++) dst[i] = (m_Lower <= src[i] && src[i] <= m_Upper) ? m_Inside : m_Outside;
  }

  InputPixelType m_Lower, m_Upper;
  OutputPixelType m_Inside, m_Outside;
};

}  // namespace itk
#endif
