// Monte-Carlo dropout inference (fcn8s_predict_mc; the definition is in fcn8s_hip.h): the one streaming kernel behind each sample's forward.
//   mc_accumulate_kernel : the sample's logits over [0,H)x[0,W), read through the PixMap (plain NHWC or the blocked layout of the last transposed
//                          conv, no unblocking pass), softmaxed in registers; p_s is added into the fp32 accumulator [N,H,W,C] and h(p_s) into
//                          the fp32 entropy accumulator [N,H,W].  The first sample stores, the last one writes no accumulator: it scales the
//                          sums by 1/S and writes whichever of mean softmax, int64 argmax, entropy h(mean) and mutual information
//                          max(0, h(mean) - mean_s h(p_s)) were asked for.  S = 1 (first and last) touches no accumulator.
// One thread per pixel, grid-stride loops capped at 2048 blocks, no atomics (every pixel belongs to one thread): two runs give the same bits.
#include "fcn8s_internal.h"
#include "entropy_term.h"
#include <cfloat>

namespace fcn8s {

static inline int mc_blocks(long long work)
{
    long long b = (work + 255) / 256;
    return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}
// slot of pixel (n, y, x) of the map (tta.hip's tta_slot: the inverse of slot_pixel in loss_tile.h)
static __device__ __forceinline__ long long mc_slot(const PixMap& m, int n, int y, int x)
{
    if (!m.blocked) return ((long long)n * m.H + y) * m.W + x;
    const int S = m.S, oy = y + S / 2, ox = x + S / 2;
    return ((((long long)n * m.QH + oy / S) * m.QW + ox / S) * S + oy % S) * S + ox % S;
}
// mc_h_add, the one term of the entropy, lives in entropy_term.h (temperature.hip folds h of a calibrated distribution through it too)

struct McGeom {
    PixMap map; int N, H, W;
    int first, last; float inv;
};
static __device__ __forceinline__ const float* mc_row(const McGeom& g, long long p, const float* logits, int C)
{
    const int x = (int)(p % g.W); const long long t = p / g.W;
    return logits + mc_slot(g.map, (int)(t / g.H), (int)(t % g.H), x) * C;
}

// C % 4 == 0 in registers: 16-byte loads / stores (softmax as softmax_argmax_kernel_c: v_i = expf(l_i - max) / sum)
template <int C>
__global__ __launch_bounds__(256) void mc_accumulate_kernel_c(const float* __restrict__ logits, const McGeom g, float* __restrict__ acc, float* __restrict__ eacc,
                                                              float* __restrict__ sm, long long* __restrict__ am, float* __restrict__ ent, float* __restrict__ mi)
{
    const long long total = (long long)g.N * g.H * g.W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
        const float4* q = reinterpret_cast<const float4*>(mc_row(g, p, logits, C));
        float v[C];
#pragma unroll
        for (int i = 0; i < C / 4; ++i) { const float4 a = q[i]; v[4*i] = a.x; v[4*i+1] = a.y; v[4*i+2] = a.z; v[4*i+3] = a.w; }
        float m = v[0];
#pragma unroll
        for (int i = 1; i < C; ++i) m = fmaxf(m, v[i]);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < C; ++i) { v[i] = expf(v[i] - m); s += v[i]; }
        float hs = 0.f;
#pragma unroll
        for (int i = 0; i < C; ++i) { v[i] = v[i] / s; hs = mc_h_add(hs, v[i]); }
        float4* ap = reinterpret_cast<float4*>(acc + p * C);
        if (!g.first) {
#pragma unroll
            for (int i = 0; i < C / 4; ++i) { const float4 t = ap[i]; v[4*i] = t.x + v[4*i]; v[4*i+1] = t.y + v[4*i+1]; v[4*i+2] = t.z + v[4*i+2]; v[4*i+3] = t.w + v[4*i+3]; }
            hs = eacc[p] + hs;
        }
        if (!g.last) {
#pragma unroll
            for (int i = 0; i < C / 4; ++i) ap[i] = make_float4(v[4*i], v[4*i+1], v[4*i+2], v[4*i+3]);
            eacc[p] = hs;
            continue;
        }
        int best = 0; float bv = -1.f, hm = 0.f;
#pragma unroll
        for (int i = 0; i < C; ++i) { v[i] = v[i] * g.inv; hm = mc_h_add(hm, v[i]); if (v[i] > bv) { bv = v[i]; best = i; } }
        if (sm) {
            float4* dst = reinterpret_cast<float4*>(sm + p * C);
#pragma unroll
            for (int i = 0; i < C / 4; ++i) dst[i] = make_float4(v[4*i], v[4*i+1], v[4*i+2], v[4*i+3]);
        }
        if (am) am[p] = best;
        if (ent) ent[p] = hm;
        if (mi) mi[p] = fmaxf(0.f, hm - hs * g.inv);
    }
}
// any C: the softmax is formed again in each sweep (max, sum, output)
__global__ __launch_bounds__(256) void mc_accumulate_kernel(const float* __restrict__ logits, const McGeom g, int C, float* __restrict__ acc, float* __restrict__ eacc,
                                                            float* __restrict__ sm, long long* __restrict__ am, float* __restrict__ ent, float* __restrict__ mi)
{
    const long long total = (long long)g.N * g.H * g.W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
        const float* q = mc_row(g, p, logits, C);
        float m = q[0];
        for (int i = 1; i < C; ++i) m = fmaxf(m, q[i]);
        float s = 0.f;
        for (int i = 0; i < C; ++i) s += expf(q[i] - m);
        float* ap = acc + p * C;
        int best = 0; float bv = -1.f, hs = 0.f, hm = 0.f;
        for (int i = 0; i < C; ++i) {
            float v = expf(q[i] - m) / s;
            hs = mc_h_add(hs, v);
            if (!g.first) v = ap[i] + v;
            if (!g.last) { ap[i] = v; continue; }
            v = v * g.inv;
            hm = mc_h_add(hm, v);
            if (sm) sm[p * C + i] = v;
            if (v > bv) { bv = v; best = i; }
        }
        if (!g.first) hs = eacc[p] + hs;
        if (!g.last) { eacc[p] = hs; continue; }
        if (am) am[p] = best;
        if (ent) ent[p] = hm;
        if (mi) mi[p] = fmaxf(0.f, hm - hs * g.inv);
    }
}

void launch_mc_accumulate(const float* logits, const PixMap& map, int N, int H, int W, int C, float* acc, float* ent_acc, int first, int last,
                          int nsamples, float* softmax_out, long long* argmax_out, float* entropy_out, float* mi_out, hipStream_t s)
{
    McGeom g;
    g.map = map; g.N = N; g.H = H; g.W = W; g.first = first; g.last = last; g.inv = 1.f / (float)nsamples;
    const int blocks = mc_blocks((long long)N * H * W);
    if (C == 20) hipLaunchKernelGGL(mc_accumulate_kernel_c<20>, dim3(blocks), dim3(256), 0, s, logits, g, acc, ent_acc, softmax_out, argmax_out, entropy_out, mi_out);
    else if (C == 4) hipLaunchKernelGGL(mc_accumulate_kernel_c<4>, dim3(blocks), dim3(256), 0, s, logits, g, acc, ent_acc, softmax_out, argmax_out, entropy_out, mi_out);
    else hipLaunchKernelGGL(mc_accumulate_kernel, dim3(blocks), dim3(256), 0, s, logits, g, C, acc, ent_acc, softmax_out, argmax_out, entropy_out, mi_out);
}

}  // namespace fcn8s
