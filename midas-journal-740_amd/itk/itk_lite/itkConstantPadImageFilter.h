// ITK-lite: itk::ConstantPadImageFilter, RESTATED from ITK's documented behaviour (no ITK source text): the output's
// region is the input's grown by the lower pad below and the upper pad above every axis -- its start index moves DOWN by the
// lower pad -- origin, spacing and direction are copied, pixels inside the input's region are the input's and every other
// pixel is the constant (default: NumericTraits<PixelType>::Zero).  Enough of the class for the recipe the reference's
// class comment prescribes -- pad by one pixel, then filter -- to be written and compared in C++ (tests/pad_update.cxx).
#ifndef ITK_LITE_itkConstantPadImageFilter_H
#define ITK_LITE_itkConstantPadImageFilter_H
#include "itkLite.h"

namespace itk {

template <class TInputImage, class TOutputImage> class ConstantPadImageFilter : public ProcessObject {
public:
  typedef ConstantPadImageFilter Self;
  typedef SmartPointer<Self> Pointer;
  itkNewMacro(Self);
  itkTypeMacro(ConstantPadImageFilter, PadImageFilter);
  typedef TInputImage InputImageType;
  typedef TOutputImage OutputImageType;
  typedef typename TOutputImage::PixelType OutputImagePixelType;
  typedef typename TInputImage::SizeType SizeType;
  static const unsigned int ImageDimension = TInputImage::ImageDimension;

  void SetInput(const TInputImage *image) { this->SetNthInput(0, const_cast<TInputImage *>(image)); }
  TOutputImage *GetOutput() { return static_cast<TOutputImage *>(this->m_Output.GetPointer()); }
  void SetConstant(OutputImagePixelType c) { m_Constant = c; this->Modified(); }
  OutputImagePixelType GetConstant() const { return m_Constant; }
  void SetPadLowerBound(const unsigned long *b) { for (unsigned int i = 0; i < ImageDimension; i++) m_Lower[i] = b[i]; this->Modified(); }
  void SetPadUpperBound(const unsigned long *b) { for (unsigned int i = 0; i < ImageDimension; i++) m_Upper[i] = b[i]; this->Modified(); }
  void SetPadLowerBound(const SizeType &b) { for (unsigned int i = 0; i < ImageDimension; i++) m_Lower[i] = b[i]; this->Modified(); }
  void SetPadUpperBound(const SizeType &b) { for (unsigned int i = 0; i < ImageDimension; i++) m_Upper[i] = b[i]; this->Modified(); }
  void SetPadBound(const SizeType &b) { this->SetPadLowerBound(b); this->SetPadUpperBound(b); }

protected:
  ConstantPadImageFilter() : m_Constant(NumericTraits<OutputImagePixelType>::Zero) {
    for (unsigned int i = 0; i < ImageDimension; i++) m_Lower[i] = m_Upper[i] = 0;
    this->SetNumberOfRequiredInputs(1);
    typename TOutputImage::Pointer o = TOutputImage::New();
    this->SetPrimaryOutput(o.GetPointer());
  }

  virtual void GenerateData() {
    const TInputImage *in = static_cast<const TInputImage *>(this->m_Inputs[0].GetPointer());
    TOutputImage *out = this->GetOutput();
    const typename TInputImage::RegionType &ir = in->GetBufferedRegion();
    typename TOutputImage::RegionType region;
    typename TOutputImage::IndexType start;
    typename TOutputImage::SizeType size;
    for (unsigned int i = 0; i < ImageDimension; i++) {
      start[i] = ir.GetIndex()[i] - static_cast<long>(m_Lower[i]);
      size[i] = ir.GetSize()[i] + m_Lower[i] + m_Upper[i];
    }
    region.SetIndex(start);
    region.SetSize(size);
    out->SetRegions(region);
    out->SetSpacing(in->GetSpacing());
    out->SetOrigin(in->GetOrigin());
    out->SetDirection(in->GetDirection());
    out->FillBuffer(m_Constant);
    // the input's pixels, line by line along the first axis, at (line's position + lower pad) of the output
    const size_t lineLen = ir.GetSize()[0];
    size_t nLines = 1;
    for (unsigned int i = 1; i < ImageDimension; i++) nLines *= ir.GetSize()[i];
    const typename TInputImage::PixelType *src = in->GetBufferPointer();
    OutputImagePixelType *dst = out->GetBufferPointer();
    for (size_t line = 0; line < nLines; line++) {
      size_t rest = line, off = m_Lower[0], stride = size[0];
      for (unsigned int i = 1; i < ImageDimension; i++) {
        const size_t pos = rest % ir.GetSize()[i];
        rest /= ir.GetSize()[i];
        off += stride * (pos + m_Lower[i]);
        stride *= size[i];
      }
      for (size_t x = 0; x < lineLen; x++) dst[off + x] = static_cast<OutputImagePixelType>(src[line * lineLen + x]);
    }
  }

  OutputImagePixelType m_Constant;
  unsigned long m_Lower[ImageDimension], m_Upper[ImageDimension];
};

}  // namespace itk
#endif
