// Test-time augmentation (fcn8s_predict_tta): the two HBM-bound kernels around each pass's forward.
//   tta_input_kernel      : uint8 / float32 RGB [N,H,W,3] -> the forward's preprocessed input x0 [N,Hp,Wp,4]: cv2 INTER_LINEAR resize
//                           to Hs x Ws (cv_resize.h, the arithmetic of resample_u8_kernel), mirror (x -> Ws-1-x), BGR mean subtraction
//                           (preprocess_kernel's), zero pad (= the VGG mean colour) to Hp x Wp.
//   tta_accumulate_kernel : the pass's logits over [0,Hs)x[0,Ws), read through the PixMap (the blocked layout of the last transposed
//                           conv, no unblocking pass), un-mirrored, resized to H x W with half-pixel centres (F.interpolate bilinear,
//                           align_corners=False), softmaxed and added into the fp32 accumulator [N,H,W,C]; the first pass stores, the
//                           last one scales the sum by 1/P and writes the softmax or the int64 argmax instead of the accumulator.
// One thread per output pixel, grid-stride loops capped at 2048 blocks, no atomics (every pixel belongs to one thread).
#include "fcn8s_internal.h"
#include "cv_resize.h"

namespace fcn8s {

static inline int tta_blocks(long long work)
{
    long long b = (work + 255) / 256;
    return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

template <int DT>      // 0: uint8, 1: float32 (no resize: Hs = H, Ws = W)
__global__ __launch_bounds__(256) void tta_input_kernel(const void* __restrict__ img, int N, int H, int W, int Hs, int Ws, int Hp, int Wp,
                                                        int flip, float4* __restrict__ out)
{
    const float m0 = 103.939f, m1 = 116.779f, m2 = 123.68f;
    const long long total = (long long)N * Hp * Wp;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wp); const long long t = i / Wp;
        const int y = (int)(t % Hp), n = (int)(t / Hp);
        if (y >= Hs || x >= Ws) { out[i] = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
        const int sx = flip ? Ws - 1 - x : x;
        float r, g, b;
        if (DT == 0) {
            int rgb[3];
            cv_resize_linear_px((const unsigned char*)img + (long long)n * H * W * 3, H, W, Hs, Ws, y, sx, rgb);
            r = (float)rgb[0]; g = (float)rgb[1]; b = (float)rgb[2];
        } else {
            const float* q = (const float*)img + (((long long)n * H + y) * W + sx) * 3;
            r = q[0]; g = q[1]; b = q[2];
        }
        out[i] = make_float4(b - m0, g - m1, r - m2, 0.f);
    }
}

void launch_tta_input(const void* img, int dtype, int N, int H, int W, int Hs, int Ws, int Hp, int Wp, int flip, float* out4, hipStream_t s)
{
    const int blocks = tta_blocks((long long)N * Hp * Wp);
    if (dtype == 0) hipLaunchKernelGGL(tta_input_kernel<0>, dim3(blocks), dim3(256), 0, s, img, N, H, W, Hs, Ws, Hp, Wp, flip, (float4*)out4);
    else hipLaunchKernelGGL(tta_input_kernel<1>, dim3(blocks), dim3(256), 0, s, img, N, H, W, Hs, Ws, Hp, Wp, flip, (float4*)out4);
}

// half-pixel source taps of output index d (torch's area_pixel_compute_source_index, align_corners = False):
// r = max((d + 0.5) src / dst - 0.5, 0), i0 = floor(r), i1 = min(i0 + 1, src - 1), weight of i1 = r - i0.  r is the exact rational
// ((2d + 1) src - dst) / (2 dst), divided in fp64 (exact floor, one rounding of the weight to fp32; an fp32 scale factor would move r by up
// to ~1e-6 at d ~ 1000, a 64-bit integer division costs more than the rest of the kernel)
struct HalfTap { int i0, i1; float l0, l1; };
static __device__ __forceinline__ HalfTap half_pixel_tap(int d, int src, int dst)
{
    long long num = (2LL * d + 1) * src - dst;
    if (num < 0) num = 0;
    const double r = (double)num / (double)(2LL * dst);
    int i0 = (int)r;
    double l = r - (double)i0;
    if (i0 > src - 1) { i0 = src - 1; l = 0.0; }
    HalfTap t; t.i0 = i0; t.i1 = i0 < src - 1 ? i0 + 1 : i0;
    t.l1 = (float)l; t.l0 = 1.f - t.l1;
    return t;
}
// slot of pixel (n, y, x) of the padded map (PixMap: map.H x map.W pixels; blocked: rows (n, q, qx) of S x S blocks that start at
// (S q - S/2, S qx - S/2), columns (r, rx, class) -- the inverse of slot_pixel in loss_tile.h)
static __device__ __forceinline__ long long tta_slot(const PixMap& m, int n, int y, int x)
{
    if (!m.blocked) return ((long long)n * m.H + y) * m.W + x;
    const int S = m.S, oy = y + S / 2, ox = x + S / 2;
    return ((((long long)n * m.QH + oy / S) * m.QW + ox / S) * S + oy % S) * S + ox % S;
}

struct TtaGeom {
    PixMap map; int N, Hs, Ws, flip, H, W;
    int first, last; float inv;
};
// the four logit rows of output pixel p (un-mirrored on a flipped pass) and the weights that combine them
static __device__ __forceinline__ void tta_taps(const TtaGeom& g, long long p, const float* logits, int C,
                                                const float* q[4], float w[4])
{
    const int x = (int)(p % g.W); const long long t = p / g.W;
    const int y = (int)(t % g.H), n = (int)(t / g.H);
    const HalfTap ty = half_pixel_tap(y, g.Hs, g.H), tx = half_pixel_tap(x, g.Ws, g.W);
    const int x0 = g.flip ? g.Ws - 1 - tx.i0 : tx.i0, x1 = g.flip ? g.Ws - 1 - tx.i1 : tx.i1;
    q[0] = logits + tta_slot(g.map, n, ty.i0, x0) * C; q[1] = logits + tta_slot(g.map, n, ty.i0, x1) * C;
    q[2] = logits + tta_slot(g.map, n, ty.i1, x0) * C; q[3] = logits + tta_slot(g.map, n, ty.i1, x1) * C;
    w[0] = ty.l0; w[1] = ty.l1; w[2] = tx.l0; w[3] = tx.l1;
}
// h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d), torch's order of operations
static __device__ __forceinline__ float bilin(const float w[4], float a, float b, float c, float d)
{
    return w[0] * (w[2] * a + w[3] * b) + w[1] * (w[2] * c + w[3] * d);
}

// C % 4 == 0 in registers: 16-byte loads / stores (softmax as softmax_argmax_kernel_c: v_i = expf(l_i - max) / sum)
template <int C>
__global__ __launch_bounds__(256) void tta_accumulate_kernel_c(const float* __restrict__ logits, const TtaGeom g, float* __restrict__ acc,
                                                               float* __restrict__ sm, long long* __restrict__ am)
{
    const long long total = (long long)g.N * g.H * g.W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
        const float* q[4]; float w[4];
        tta_taps(g, p, logits, C, q, w);
        float v[C];
#pragma unroll
        for (int i = 0; i < C / 4; ++i) {
            const float4 a = reinterpret_cast<const float4*>(q[0])[i], b = reinterpret_cast<const float4*>(q[1])[i];
            const float4 c = reinterpret_cast<const float4*>(q[2])[i], d = reinterpret_cast<const float4*>(q[3])[i];
            v[4*i] = bilin(w, a.x, b.x, c.x, d.x); v[4*i+1] = bilin(w, a.y, b.y, c.y, d.y);
            v[4*i+2] = bilin(w, a.z, b.z, c.z, d.z); v[4*i+3] = bilin(w, a.w, b.w, c.w, d.w);
        }
        float m = v[0];
#pragma unroll
        for (int i = 1; i < C; ++i) m = fmaxf(m, v[i]);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < C; ++i) { v[i] = expf(v[i] - m); s += v[i]; }
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = v[i] / s;
        float4* ap = reinterpret_cast<float4*>(acc + p * C);
        if (!g.first) {
#pragma unroll
            for (int i = 0; i < C / 4; ++i) { const float4 t = ap[i]; v[4*i] = t.x + v[4*i]; v[4*i+1] = t.y + v[4*i+1]; v[4*i+2] = t.z + v[4*i+2]; v[4*i+3] = t.w + v[4*i+3]; }
        }
        if (!g.last) {
#pragma unroll
            for (int i = 0; i < C / 4; ++i) ap[i] = make_float4(v[4*i], v[4*i+1], v[4*i+2], v[4*i+3]);
            continue;
        }
        int best = 0; float bv = -1.f;
#pragma unroll
        for (int i = 0; i < C; ++i) { v[i] = v[i] * g.inv; if (v[i] > bv) { bv = v[i]; best = i; } }
        if (sm) {
            float4* dst = reinterpret_cast<float4*>(sm + p * C);
#pragma unroll
            for (int i = 0; i < C / 4; ++i) dst[i] = make_float4(v[4*i], v[4*i+1], v[4*i+2], v[4*i+3]);
        }
        if (am) am[p] = best;
    }
}
// any C: the interpolated logits are formed again in each of the three sweeps (max, sum, output)
__global__ __launch_bounds__(256) void tta_accumulate_kernel(const float* __restrict__ logits, const TtaGeom g, int C, float* __restrict__ acc,
                                                             float* __restrict__ sm, long long* __restrict__ am)
{
    const long long total = (long long)g.N * g.H * g.W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
        const float* q[4]; float w[4];
        tta_taps(g, p, logits, C, q, w);
        float m = bilin(w, q[0][0], q[1][0], q[2][0], q[3][0]);
        for (int i = 1; i < C; ++i) m = fmaxf(m, bilin(w, q[0][i], q[1][i], q[2][i], q[3][i]));
        float s = 0.f;
        for (int i = 0; i < C; ++i) s += expf(bilin(w, q[0][i], q[1][i], q[2][i], q[3][i]) - m);
        float* ap = acc + p * C;
        int best = 0; float bv = -1.f;
        for (int i = 0; i < C; ++i) {
            float v = expf(bilin(w, q[0][i], q[1][i], q[2][i], q[3][i]) - m) / s;
            if (!g.first) v = ap[i] + v;
            if (!g.last) { ap[i] = v; continue; }
            v = v * g.inv;
            if (sm) sm[p * C + i] = v;
            if (v > bv) { bv = v; best = i; }
        }
        if (g.last && am) am[p] = best;
    }
}

void launch_tta_accumulate(const float* logits, const PixMap& map, int N, int Hs, int Ws, int flip, int C, int H, int W, float* acc,
                           int first, int last, int npasses, float* softmax_out, long long* argmax_out, hipStream_t s)
{
    TtaGeom g;
    g.map = map; g.N = N; g.Hs = Hs; g.Ws = Ws; g.flip = flip; g.H = H; g.W = W;
    g.first = first; g.last = last; g.inv = 1.f / (float)npasses;
    const int blocks = tta_blocks((long long)N * H * W);
    if (C == 20) hipLaunchKernelGGL(tta_accumulate_kernel_c<20>, dim3(blocks), dim3(256), 0, s, logits, g, acc, softmax_out, argmax_out);
    else if (C == 4) hipLaunchKernelGGL(tta_accumulate_kernel_c<4>, dim3(blocks), dim3(256), 0, s, logits, g, acc, softmax_out, argmax_out);
    else hipLaunchKernelGGL(tta_accumulate_kernel, dim3(blocks), dim3(256), 0, s, logits, g, C, acc, softmax_out, argmax_out);
}

}  // namespace fcn8s
