// cross_core.h -- the two expressions of the cross-spectrum front end (include/rpf_engine.h,
// rpf_accumulate_device_cross): the combined streams u = a + b and v = a + i b, sample by sample, and the finishing
// expression that turns the four power planes into Saa, Sbb, Re Sab, Im Sab.  Every operation is rounded on its own;
// nothing is contracted or reassociated.  The sample conversion is pfb_core.h's (cu8: v - 127; cs8, cs16, cf32: v).
//
// Plain C++: the kernels (rpf_cross.hip) and the CPU tests (tests/emul/cross_emul.cpp) share what is below, so the two
// cannot drift.
#pragma once

#include "pfb_core.h"

namespace rpf {

constexpr int kCrossPlanes = 4;     // in: Paa, Pbb, Puu, Pvv; out: Saa, Sbb, Re Sab, Im Sab

// u = (aI + bI, aQ + bQ) = a + b;  v = (aI - bQ, aQ + bI) = a + i b.  One float32 rounding per component: exact for the
// three integer formats (sums of 16-bit values are float32 integers).
RPF_PFB_HD void cross_combine_sample(float aI, float aQ, float bI, float bQ, float (&u)[2], float (&v)[2])
{
#pragma clang fp contract(off)
    u[0] = aI + bI;
    u[1] = aQ + bQ;
    v[0] = aI - bQ;
    v[1] = aQ + bI;
}

// C = Paa + Pbb;  out = Paa, Pbb, 0.5 (Puu - C), 0.5 (Pvv - C), in double, in exactly this order.
RPF_PFB_HD void cross_finish_bin(double paa, double pbb, double puu, double pvv, double (&out)[kCrossPlanes])
{
#pragma clang fp contract(off)
    const double c = paa + pbb;
    out[0] = paa;
    out[1] = pbb;
    out[2] = 0.5 * (puu - c);
    out[3] = 0.5 * (pvv - c);
}

}  // namespace rpf
