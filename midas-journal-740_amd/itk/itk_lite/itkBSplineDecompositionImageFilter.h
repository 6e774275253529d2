// ITK-lite forwarding header: carries the ITK file name, the declarations live in itkBSplineLite.h
#ifndef ITK_LITE_FWD_itkBSplineDecompositionImageFilter_H
#define ITK_LITE_FWD_itkBSplineDecompositionImageFilter_H
#include "itkBSplineLite.h"
#endif
