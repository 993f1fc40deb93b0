// The update's own HBM-bound kernels (definitions: include/fcn8s_hip.h, "the update"): folding a gradient bucket into the accumulator and
// flushing it back, the global norm of the flat gradient buffer in a fixed summation order, and the TF-Adam / SGD-momentum kernels that
// read their gradient scale and the guard's verdict from device memory.  16-byte accesses, grid-stride loops capped at 2048 blocks.
#include "fcn8s_internal.h"
#include <math.h>

namespace fcn8s {

static inline int cap_blocks(long long work, int per_block)
{
    long long b = (work + per_block - 1) / per_block;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

// a float4 at a 4-byte aligned address (a bucket sub-range, an op-level pointer): one 16-byte access all the same
struct __attribute__((packed, aligned(4))) float4_u { float x, y, z, w; };

// floats in front of the first 16-byte aligned element of p (at most n)
static inline long long head_floats(const void* p, long long n)
{
    const long long h = (long long)((4 - (((uintptr_t)p >> 2) & 3)) & 3);
    return h < n ? h : n;
}

// ---- fold / flush: dst = src (MODE 0) or dst = dst + src (MODE 1) over [0, n) --------------------------------------------------------------
// dst + head is 16-byte aligned; the body is n4 float4 from there; head and tail (< 4 floats each) are scalar.  SRC_ALIGNED: src + head is
// 16-byte aligned too (what a model's buckets are: acc and the gradient buffer share their offsets).
template <int MODE, bool SRC_ALIGNED>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ dst, const float* __restrict__ src, long long head, long long n4, long long n)
{
    const long long gtid = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    float4* d4 = (float4*)(dst + head);
    for (long long i = gtid; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 a;
        if (SRC_ALIGNED) a = ((const float4*)(src + head))[i];
        else { const float4_u u = ((const float4_u*)(src + head))[i]; a = make_float4(u.x, u.y, u.z, u.w); }
        if (MODE == 1) { const float4 b = d4[i]; a.x = b.x + a.x; a.y = b.y + a.y; a.z = b.z + a.z; a.w = b.w + a.w; }
        d4[i] = a;
    }
    const long long tail0 = head + n4 * 4;
    long long j = -1;
    if (gtid < head) j = gtid;
    else if (gtid - head < n - tail0) j = tail0 + (gtid - head);
    if (j >= 0) dst[j] = MODE == 1 ? dst[j] + src[j] : src[j];
}

void launch_grad_accumulate(float* dst, const float* src, long long n, int mode, hipStream_t s)
{
    if (n <= 0) return;
    const long long head = head_floats(dst, n), n4 = (n - head) / 4;
    const bool al = (((uintptr_t)(src + head)) & 15) == 0;
    const dim3 grid(cap_blocks(n4, 256)), block(256);          // (one block at least: the 3 + 3 scalar lanes)
#define GA(M, A) hipLaunchKernelGGL((grad_accumulate_kernel<M, A>), grid, block, 0, s, dst, src, head, n4, n)
    if (mode == 0) { if (al) GA(0, true); else GA(0, false); }
    else           { if (al) GA(1, true); else GA(1, false); }
#undef GA
}

// ---- the global norm ----------------------------------------------------------------------------------------------------------------------
// lanes by a shuffle tree, waves in index order; the result is valid in thread 0
static __device__ __forceinline__ double norm_block_sum(double v, double* sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double t = 0;
    if (threadIdx.x == 0) for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
    return t;
}

// partials[block] = the block's share of sum (double)g^2: lane (block, thread) takes float4 number block * 256 + thread, then every
// (gridDim * 256)-th one, components in order; the scalar head and tail go to the first lanes of the grid.  Always kGradNormBlocks blocks.
__global__ __launch_bounds__(256) void grad_sumsq_partials_kernel(const float* __restrict__ g, long long head, long long n4, long long n, double* __restrict__ partials)
{
    __shared__ double sh[4];
    const long long gtid = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const float4* g4 = (const float4*)(g + head);
    double v = 0;
    for (long long i = gtid; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 a = g4[i];
        v += (double)a.x * (double)a.x; v += (double)a.y * (double)a.y; v += (double)a.z * (double)a.z; v += (double)a.w * (double)a.w;
    }
    const long long tail0 = head + n4 * 4;
    if (gtid < head) v += (double)g[gtid] * (double)g[gtid];
    else if (gtid - head < n - tail0) { const float x = g[tail0 + (gtid - head)]; v += (double)x * (double)x; }
    const double t = norm_block_sum(v, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// one block: S = the slab in index order (lane t: entries 8t .. 8t + 7, then the tree), then the clip's five numbers
template <bool AS_FLOATS>
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const double* __restrict__ partials, float grad_scale, float max_norm, void* out)
{
    __shared__ double sh[4];
    constexpr int per = kGradNormBlocks / 256;
    double v = 0;
    for (int i = 0; i < per; ++i) v += partials[threadIdx.x * per + i];
    const double S = norm_block_sum(v, sh);
    if (threadIdx.x != 0) return;
    const float norm = (float)((double)fabsf(grad_scale) * sqrt(S));
    // (max_norm = 0: no clip; +inf: the guard alone, inf / inf is not asked; fmaxf(NaN, x) = x: a NaN norm leaves c = 1, and ok = 0)
    const float c = (max_norm > 0.f && !isinf(max_norm)) ? max_norm / fmaxf(norm, max_norm) : 1.f;
    const float sc = grad_scale * c;
    const bool ok = isfinite(norm);
    if (AS_FLOATS) {
        float* o = (float*)out;
        o[0] = norm; o[1] = c; o[2] = sc; o[3] = ok ? 1.f : 0.f; o[4] = 0.f;
    } else {
        UpdateStats* o = (UpdateStats*)out;
        o->norm = norm; o->clip = c; o->scale = sc; o->ok = ok ? 1 : 0;
        if (!ok) o->skipped += 1;
    }
}

void launch_grad_norm(const float* g, long long n, float grad_scale, float max_norm, double* partials, void* out, bool as_floats, hipStream_t s)
{
    if (n < 0) n = 0;
    const long long head = head_floats(g, n), n4 = (n - head) / 4;
    hipLaunchKernelGGL(grad_sumsq_partials_kernel, dim3(kGradNormBlocks), dim3(256), 0, s, g, head, n4, n, partials);
    if (as_floats) hipLaunchKernelGGL(grad_norm_finalize_kernel<true>, dim3(1), dim3(256), 0, s, (const double*)partials, grad_scale, max_norm, out);
    else           hipLaunchKernelGGL(grad_norm_finalize_kernel<false>, dim3(1), dim3(256), 0, s, (const double*)partials, grad_scale, max_norm, out);
}

// ---- the optimizers of elementwise.hip (K12) with the gradient scale and the guard's verdict read from the device ---------------------------
// the same expressions as tf_adam_kernel / sgd_momentum_kernel: with *s_dev == gs they give the same bits
__global__ __launch_bounds__(256) void tf_adam_dev_kernel(float4* theta, const float4* g, float4* m, float4* v,
                                                          long long n4, float lr_t, float b1, float b2, float eps,
                                                          const float* __restrict__ s_dev, const int* __restrict__ ok_dev)
{
    if (*ok_dev == 0) return;
    const float gs = *s_dev;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 t = theta[i], gg = g[i], mm = m[i], vv = v[i];
#define ADAM1(F) { const float gr = gg.F * gs; mm.F = b1 * mm.F + (1.f - b1) * gr; vv.F = b2 * vv.F + (1.f - b2) * gr * gr; \
                   t.F -= lr_t * mm.F / (sqrtf(vv.F) + eps); }
        ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
#undef ADAM1
        theta[i] = t; m[i] = mm; v[i] = vv;
    }
}
__global__ void tf_adam_dev_tail_kernel(float* theta, const float* g, float* m, float* v, long long n0, long long n,
                                        float lr_t, float b1, float b2, float eps, const float* __restrict__ s_dev, const int* __restrict__ ok_dev)
{
    if (*ok_dev == 0) return;
    const float gs = *s_dev;
    const long long i = n0 + threadIdx.x;
    if (i < n) {
        const float gr = g[i] * gs;
        m[i] = b1 * m[i] + (1.f - b1) * gr; v[i] = b2 * v[i] + (1.f - b2) * gr * gr;
        theta[i] -= lr_t * m[i] / (sqrtf(v[i]) + eps);
    }
}
void launch_tf_adam_dev(float* theta, const float* g, float* m, float* v, long long n,
                        float lr_t, float b1, float b2, float eps, const float* s_dev, const int* ok_dev, hipStream_t s)
{
    const long long n4 = n / 4;
    if (n4 > 0)
        hipLaunchKernelGGL(tf_adam_dev_kernel, dim3(cap_blocks(n4, 256)), dim3(256), 0, s, (float4*)theta, (const float4*)g,
                           (float4*)m, (float4*)v, n4, lr_t, b1, b2, eps, s_dev, ok_dev);
    if (n4 * 4 < n)
        hipLaunchKernelGGL(tf_adam_dev_tail_kernel, dim3(1), dim3(4), 0, s, theta, g, m, v, n4 * 4, n, lr_t, b1, b2, eps, s_dev, ok_dev);
}
__global__ __launch_bounds__(256) void sgd_momentum_dev_kernel(float* theta, const float* g, float* buf, long long n,
                                                               float lr, float mom, const float* __restrict__ s_dev, const int* __restrict__ ok_dev)
{
    if (*ok_dev == 0) return;
    const float gs = *s_dev;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float b = mom * buf[i] + g[i] * gs;
        buf[i] = b;
        theta[i] -= lr * b;
    }
}
void launch_sgd_momentum_dev(float* theta, const float* g, float* buf, long long n, float lr, float mom,
                             const float* s_dev, const int* ok_dev, hipStream_t s)
{
    hipLaunchKernelGGL(sgd_momentum_dev_kernel, dim3(cap_blocks(n, 256)), dim3(256), 0, s, theta, g, buf, n, lr, mom, s_dev, ok_dev);
}

}  // namespace fcn8s
