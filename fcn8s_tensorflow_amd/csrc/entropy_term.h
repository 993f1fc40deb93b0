// The entropy's one device function, shared by mc_dropout.hip (h(p_s), h(mean)) and temperature.hip (h of the calibrated distribution).
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

namespace fcn8s {

// One term of h(p) = -sum_c p_c logf(max(p_c, FLT_MIN)), added to the running sum.  THE one place the entropy's arithmetic is written: h(p_s) and
// h(mean) both fold their classes through it in class order, with contraction off, so the same p gives the same bits in both places (the
// identity "no dropout -> mutual information == 0.0" rests on that: a multiply-add contracted in one inlined copy and not in the other breaks it).
static __device__ __forceinline__ float mc_h_add(float h, float p)
{
#pragma clang fp contract(off)
    const float t = p * logf(fmaxf(p, FLT_MIN));
    return h - t;
}

}  // namespace fcn8s
