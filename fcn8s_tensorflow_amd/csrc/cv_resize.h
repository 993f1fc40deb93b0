// cv2.resize on 8-bit RGB data in OpenCV's own arithmetic (restated from resize.cpp in fcn8s_tensorflow_amd/cv2_compat.py, which these
// functions match bit for bit).  Shared by resample_u8_kernel (elementwise.hip) and tta_input_kernel (tta.hip).
// INTER_LINEAR: f = float((d + 0.5) * scale - 0.5) with scale = 1 / (dst / src) in double; s = floor(f); f -= s; columns clamp s and zero f
// at the borders, rows clamp the two row numbers; taps rounded to 11-bit fixed point; horizontal pass in int32; vertical pass
// (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.  An exact 2x shrink in both directions is the 2x2 box mean (INTER_AREA).
// INTER_NEAREST: s = min(floor(d * (1 / (dst / src))), src - 1).
#pragma once
#include <hip/hip_runtime.h>

namespace fcn8s {

struct CvTap { int s; int w0, w1; };
static __device__ __forceinline__ CvTap cv_linear_tap(int d, int src, int dst, bool clamp_index)
{
    const double scale = 1.0 / ((double)dst / (double)src);
    float f = (float)__dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5);
    int s = (int)floorf(f);
    f = __fsub_rn(f, (float)s);
    if (clamp_index) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= src - 1) { f = 0.f; s = src - 1; }
    }
    CvTap t; t.s = s;
    t.w0 = (int)rintf(__fmul_rn(__fsub_rn(1.f, f), 2048.f)); t.w1 = (int)rintf(__fmul_rn(f, 2048.f));
    return t;
}
static __device__ __forceinline__ int cv_nearest_index(int d, int src, int dst)
{
    const double ifx = 1.0 / ((double)dst / (double)src);
    const int s = (int)floor(__dmul_rn((double)d, ifx));
    return s < src - 1 ? s : src - 1;
}
// pixel (ry, rx) of the H x W RGB image at `base` resized to rh x rw (INTER_LINEAR; 0 <= ry < rh, 0 <= rx < rw): the three channels
static __device__ __forceinline__ void cv_resize_linear_px(const unsigned char* __restrict__ base, int H, int W, int rh, int rw, int ry, int rx, int rgb[3])
{
    if (rh == H && rw == W) {
        const long long src = ((long long)ry * W + rx) * 3;
        rgb[0] = base[src]; rgb[1] = base[src + 1]; rgb[2] = base[src + 2];
        return;
    }
    if (H == 2 * rh && W == 2 * rw) {
        const unsigned char* p0 = base + ((long long)(2 * ry) * W + 2 * rx) * 3;
        const unsigned char* p1 = p0 + (long long)W * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = ((int)p0[c] + p0[3 + c] + p1[c] + p1[3 + c] + 2) >> 2;
        return;
    }
    const CvTap tx = cv_linear_tap(rx, W, rw, true), ty = cv_linear_tap(ry, H, rh, false);
    const int x1 = tx.s + 1 < W ? tx.s + 1 : W - 1;                       // (weight 0 there)
    const int r0 = ty.s < 0 ? 0 : (ty.s >= H ? H - 1 : ty.s), r1 = ty.s + 1 < 0 ? 0 : (ty.s + 1 >= H ? H - 1 : ty.s + 1);
    const unsigned char* q0 = base + (long long)r0 * W * 3;
    const unsigned char* q1 = base + (long long)r1 * W * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int S0 = (int)q0[tx.s * 3 + c] * tx.w0 + (int)q0[x1 * 3 + c] * tx.w1;
        const int S1 = (int)q1[tx.s * 3 + c] * tx.w0 + (int)q1[x1 * 3 + c] * tx.w1;
        rgb[c] = (((ty.w0 * (S0 >> 4)) >> 16) + ((ty.w1 * (S1 >> 4)) >> 16) + 2) >> 2;
    }
}

}  // namespace fcn8s
