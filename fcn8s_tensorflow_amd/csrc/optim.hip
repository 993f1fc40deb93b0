// The update's own HBM-bound kernels (definitions: include/fcn8s_hip.h, "the update"): folding a gradient bucket into the accumulator and
// flushing it back, the global norm of the flat gradient buffer in a fixed summation order, and the one TF-Adam / SGD-momentum kernel, which takes
// its gradient scale from the host or, with the guard's verdict, from device memory and folds the moving average of the parameters ("the
// average") into the same pass when there is one; the average alone, and the swap.  16-byte accesses, grid-stride loops capped at 2048 blocks
// (the update: one float4 per lane).
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

// ---- the moving average of the parameters (definitions: include/fcn8s_hip.h, "the average") -------------------------------------------------
// s <- s - w (s - theta): one subtraction and one fused multiply-add, written out so that every kernel below gives the same bits
static __device__ __forceinline__ float ema1(float s, float t, float w) { return __builtin_fmaf(-w, s - t, s); }

// ---- the update: TF-Adam / SGD-momentum, host or device gradient scale, with or without the average -- one kernel body ----------------------
// One element of the update, with every rounding written out: the bits of a training step are pinned here, not left to the compiler's choice of
// where to contract a multiply-add.  TF-Adam has two forms: FUSED folds the last product of the m and of the v update into the sum, the other
// rounds both products first.  Elements below 4 (n / 4) take the fused form, the up to three behind them the other, whatever lane computes the
// element.  SGD-momentum rounds both products of the momentum and fuses theta's.  (contract(off): a * b + c below is two roundings; the one
// rounding is spelled fmaf.  The __fmul_rn family would not do: it is plain arithmetic that the compiler contracts like any other.)
template <bool FUSED>
static __device__ __forceinline__ void adam1(float& t, float g, float& m, float& v, float lr_t, float b1, float b2, float eps, float gs)
{
#pragma clang fp contract(off)
    const float gr = g * gs, c1 = 1.f - b1, c2 = 1.f - b2;
    if (FUSED) { m = __builtin_fmaf(c1, gr, b1 * m); v = __builtin_fmaf(c2 * gr, gr, b2 * v); }
    else       { m = b1 * m + c1 * gr; v = b2 * v + (c2 * gr) * gr; }
    t -= lr_t * m / (sqrtf(v) + eps);
}
static __device__ __forceinline__ void adam1(bool fused, float& t, float g, float& m, float& v, float lr_t, float b1, float b2, float eps, float gs)
{
    if (fused) adam1<true>(t, g, m, v, lr_t, b1, b2, eps, gs); else adam1<false>(t, g, m, v, lr_t, b1, b2, eps, gs);
}
static __device__ __forceinline__ void sgd1(float& t, float g, float& buf, float lr, float mom, float gs)
{
#pragma clang fp contract(off)
    const float b = mom * buf + g * gs;
    buf = b;
    t = __builtin_fmaf(-lr, b, t);
}

template <bool ALIGNED> static __device__ __forceinline__ float4 ld4(const float* p, long long i)
{
    if (ALIGNED) return ((const float4*)p)[i];
    const float4_u u = ((const float4_u*)p)[i];
    return make_float4(u.x, u.y, u.z, u.w);
}
template <bool ALIGNED> static __device__ __forceinline__ void st4(float* p, long long i, const float4& a)
{
    if (ALIGNED) ((float4*)p)[i] = a;
    else { float4_u u; u.x = a.x; u.y = a.y; u.z = a.z; u.w = a.w; ((float4_u*)p)[i] = u; }
}
// the scalar lanes of a launch whose body is n4 float4 from `head` on: element index of this lane, or -1 (the pattern of grad_accumulate_kernel)
static __device__ __forceinline__ long long edge_lane(long long gtid, long long head, long long n4, long long n)
{
    const long long tail0 = head + n4 * 4;
    if (gtid < head) return gtid;
    if (gtid - head < n - tail0) return tail0 + (gtid - head);
    return -1;
}

// The one update kernel: theta, m (, v) of an optimizer step and, with EMA, s from the new theta while it is in registers (without: a.shadow is
// null and never read).  OPT: FCN8S_OPT_TF_ADAM (p0 .. p3 = lr_t, beta1, beta2, eps) or FCN8S_OPT_SGD_MOMENTUM (p0, p1 = lr, momentum; v unused).
// a.s_dev != nullptr: the gradient scale and the guard's verdict come from the device, and *ok_dev == 0 returns before anything else is read.
// theta + head is 16-byte aligned; ALIGNED: so are g, m, v and s at + head (a model's buffers).
template <int OPT, bool EMA, bool ALIGNED>
static __device__ __forceinline__ void update_body(const UpdateArgs& a, long long head, long long n4)
{
    float gs = a.gs;
    if (a.s_dev) { if (*a.ok_dev == 0) return; gs = *a.s_dev; }
    float* theta = a.theta; const float* g = a.g; float* m = a.m; float* v = a.v; float* s = a.shadow;
    const long long n = a.n;
    const float p0 = a.p0, p1 = a.p1, p2 = a.p2, p3 = a.p3, w = a.ema_w;
    const long long gtid = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long nb = n & ~3LL;          // Adam: the launcher ends the float4 body here, so the body is all of the fused form
    for (long long i = gtid; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 t = ((float4*)(theta + head))[i], ss;
        const float4 gg = ld4<ALIGNED>(g + head, i);
        float4 mm = ld4<ALIGNED>(m + head, i);
        if (EMA) ss = ld4<ALIGNED>(s + head, i);
        if (OPT == FCN8S_OPT_TF_ADAM) {
            float4 vv = ld4<ALIGNED>(v + head, i);
            adam1<true>(t.x, gg.x, mm.x, vv.x, p0, p1, p2, p3, gs); adam1<true>(t.y, gg.y, mm.y, vv.y, p0, p1, p2, p3, gs);
            adam1<true>(t.z, gg.z, mm.z, vv.z, p0, p1, p2, p3, gs); adam1<true>(t.w, gg.w, mm.w, vv.w, p0, p1, p2, p3, gs);
            st4<ALIGNED>(v + head, i, vv);
        } else {
            sgd1(t.x, gg.x, mm.x, p0, p1, gs); sgd1(t.y, gg.y, mm.y, p0, p1, gs);
            sgd1(t.z, gg.z, mm.z, p0, p1, gs); sgd1(t.w, gg.w, mm.w, p0, p1, gs);
        }
        ((float4*)(theta + head))[i] = t;
        st4<ALIGNED>(m + head, i, mm);
        if (EMA) {
            ss.x = ema1(ss.x, t.x, w); ss.y = ema1(ss.y, t.y, w); ss.z = ema1(ss.z, t.z, w); ss.w = ema1(ss.w, t.w, w);
            st4<ALIGNED>(s + head, i, ss);
        }
    }
    const long long j = edge_lane(gtid, head, n4, n);
    if (j >= 0) {
        float t = theta[j], mm = m[j];
        if (OPT == FCN8S_OPT_TF_ADAM) { float vv = v[j]; adam1(j < nb, t, g[j], mm, vv, p0, p1, p2, p3, gs); v[j] = vv; }
        else sgd1(t, g[j], mm, p0, p1, gs);
        theta[j] = t; m[j] = mm;
        if (EMA) s[j] = ema1(s[j], t, w);
    }
}
// (the names the profile tools know the update by)
template <bool EMA, bool ALIGNED>
__global__ __launch_bounds__(256) void tf_adam_kernel(UpdateArgs a, long long head, long long n4) { update_body<FCN8S_OPT_TF_ADAM, EMA, ALIGNED>(a, head, n4); }
template <bool EMA, bool ALIGNED>
__global__ __launch_bounds__(256) void sgd_momentum_kernel(UpdateArgs a, long long head, long long n4) { update_body<FCN8S_OPT_SGD_MOMENTUM, EMA, ALIGNED>(a, head, n4); }

void launch_update(const UpdateArgs& a, hipStream_t st)
{
    if (a.n <= 0) return;
    const bool adam = a.opt == FCN8S_OPT_TF_ADAM;
    // Adam: no float4 of the body reaches over 4 (n / 4), so the body is all of one form; up to 3 + 6 scalar lanes
    const long long n = a.n, head = head_floats(a.theta, n), nb = n & ~3LL, n4 = adam ? (nb > head ? (nb - head) / 4 : 0) : (n - head) / 4;
    auto al16 = [&](const float* p) { return p == nullptr || (((uintptr_t)(p + head)) & 15) == 0; };
    const bool al = al16(a.g) && al16(a.m) && al16(a.v) && al16(a.shadow);
    // One float4 per lane, not cap_blocks' 2048 blocks (the loop stays for a grid clipped at 2^31 - 1): at 16 bytes per lane a capped grid strides
    // 8 MB per array and iteration, and measured at the model's width that sweep runs the SGD-momentum update at 4.6 TB/s against 5.6 TB/s uncapped.
    const long long nblk = (n4 + 255) / 256;
    const dim3 grid((unsigned)(nblk < 1 ? 1 : nblk > 0x7fffffffLL ? 0x7fffffffLL : nblk)), block(256);          // (one block at least: the scalar lanes)
#define UP(K, E, A) hipLaunchKernelGGL((K<E, A>), grid, block, 0, st, a, head, n4)
#define UP2(K) do { if (a.shadow) { if (al) UP(K, true, true); else UP(K, true, false); } else { if (al) UP(K, false, true); else UP(K, false, false); } } while (0)
    if (adam) UP2(tf_adam_kernel); else UP2(sgd_momentum_kernel);
#undef UP2
#undef UP
}

// the average alone (FCN8S_OPT_NONE: the caller wrote theta): s + head is 16-byte aligned; ok_dev may be null (no guard)
template <bool ALIGNED>
__global__ __launch_bounds__(256) void ema_update_kernel(float* s, const float* __restrict__ theta, long long head, long long n4, long long n, float w,
                                                         const int* __restrict__ ok_dev)
{
    if (ok_dev && *ok_dev == 0) return;
    const long long gtid = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    for (long long i = gtid; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 ss = ((float4*)(s + head))[i];
        const float4 t = ld4<ALIGNED>(theta + head, i);
        ss.x = ema1(ss.x, t.x, w); ss.y = ema1(ss.y, t.y, w); ss.z = ema1(ss.z, t.z, w); ss.w = ema1(ss.w, t.w, w);
        ((float4*)(s + head))[i] = ss;
    }
    const long long j = edge_lane(gtid, head, n4, n);
    if (j >= 0) s[j] = ema1(s[j], theta[j], w);
}
void launch_ema_update(float* sh, const float* theta, long long n, float w, const int* ok_dev, hipStream_t st)
{
    if (n <= 0) return;
    const long long head = head_floats(sh, n), n4 = (n - head) / 4;
    const dim3 grid(cap_blocks(n4, 256)), block(256);
    if ((((uintptr_t)(theta + head)) & 15) == 0) hipLaunchKernelGGL(ema_update_kernel<true>, grid, block, 0, st, sh, theta, head, n4, n, w, ok_dev);
    else                                         hipLaunchKernelGGL(ema_update_kernel<false>, grid, block, 0, st, sh, theta, head, n4, n, w, ok_dev);
}

// a <-> b in place (fcn8s_ema_swap): a + head is 16-byte aligned; the ranges do not overlap
template <bool ALIGNED>
__global__ __launch_bounds__(256) void swap_kernel(float* a, float* b, long long head, long long n4, long long n)
{
    const long long gtid = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    for (long long i = gtid; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 x = ((float4*)(a + head))[i], y = ld4<ALIGNED>(b + head, i);
        ((float4*)(a + head))[i] = y;
        st4<ALIGNED>(b + head, i, x);
    }
    const long long j = edge_lane(gtid, head, n4, n);
    if (j >= 0) { const float x = a[j]; a[j] = b[j]; b[j] = x; }
}
void launch_swap(float* a, float* b, long long n, hipStream_t st)
{
    if (n <= 0) return;
    const long long head = head_floats(a, n), n4 = (n - head) / 4;
    const dim3 grid(cap_blocks(n4, 256)), block(256);
    if ((((uintptr_t)(b + head)) & 15) == 0) hipLaunchKernelGGL(swap_kernel<true>, grid, block, 0, st, a, b, head, n4, n);
    else                                     hipLaunchKernelGGL(swap_kernel<false>, grid, block, 0, st, a, b, head, n4, n);
}

}  // namespace fcn8s
