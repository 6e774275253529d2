// ITK-lite forwarding header: carries the ITK file name; BSplineInterpolateImageFunction (and the decomposition filter it
// runs) live in itkBSplineLite.h
#ifndef ITK_LITE_FWD_itkBSplineInterpolateImageFunction_H
#define ITK_LITE_FWD_itkBSplineInterpolateImageFunction_H
#include "itkLite.h"
#include "itkBSplineLite.h"
#endif
