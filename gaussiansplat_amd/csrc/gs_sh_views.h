// gs_sh_views.h -- the SH basis constants of the per-gaussian backward kernels.  gs_preprocess_bwd.hip defines them at file scope, as
// it always has; another translation unit of the library that includes gs_sh_views_body.inc names a namespace for them
// (GS_SH_CONSTANTS_NS before the include), or the library would define the same symbols twice.  Same values, same loads.
#pragma once
#include "gs_common.h"

#define SH_C0 0.28209479177387814f
#define SH_C1 0.48860251190291990f
#ifdef GS_SH_CONSTANTS_NS
namespace GS_SH_CONSTANTS_NS {
#endif
__constant__ float bC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                             -1.0925484305920792f, 0.5462742152960396f};
__constant__ float bC3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                             -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};
#ifdef GS_SH_CONSTANTS_NS
}
using namespace GS_SH_CONSTANTS_NS;
#endif
