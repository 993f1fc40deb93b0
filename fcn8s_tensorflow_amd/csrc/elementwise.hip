// HBM-bound kernels of the FCN-8s path: input preprocessing, 2x2 max-pool
// (forward / backward with fused ReLU mask), fused softmax-cross-entropy
// (loss + dlogits in one pass over the logits), softmax+argmax, confusion
// matrix, column sums (bias gradients), optimizer updates and the small weight
// re-layouts.  16-byte vector accesses, grid-stride loops capped at 2048 blocks.
#include "fcn8s_internal.h"
#include "loss_tile.h"
#include "cv_resize.h"
#include <math.h>
#include <map>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>

namespace fcn8s {

static inline int cap_blocks(long long work, int per_block)
{
    long long b = (work + per_block - 1) / per_block;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

// ---- K0: uint8/float RGB -> float BGR - mean, padded to 4 channels ---------
__global__ void preprocess_kernel(const void* img, int dtype, float4* out, long long npix)
{
    const float m0 = 103.939f, m1 = 116.779f, m2 = 123.68f;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix;
         p += (long long)gridDim.x * blockDim.x) {
        float r, g, b;
        if (dtype == 0) {
            const uint8_t* q = (const uint8_t*)img + p * 3;
            r = q[0]; g = q[1]; b = q[2];
        } else {
            const float* q = (const float*)img + p * 3;
            r = q[0]; g = q[1]; b = q[2];
        }
        out[p] = make_float4(b - m0, g - m1, r - m2, 0.f);
    }
}
void launch_preprocess(const void* img, int dtype, float* out4, long long npix, hipStream_t s)
{
    hipLaunchKernelGGL(preprocess_kernel, dim3(cap_blocks(npix, 256)), dim3(256), 0, s, img, dtype,
                       (float4*)out4, npix);
}

// ---- K2: max-pool 2x2/2 (C % 4 == 0, H,W even) ------------------------------
__global__ void maxpool_fwd_kernel(const float4* x, float4* y, int N, int H, int W, int C4)
{
    const int Ho = H / 2, Wo = W / 2;
    const long long total = (long long)N * Ho * Wo * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long t = i / C4;
        const int w = (int)(t % Wo); t /= Wo;
        const int h = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const long long base = (((long long)n * H + 2 * h) * W + 2 * w) * C4 + c;
        const float4 a = x[base], b = x[base + C4], cc = x[base + (long long)W * C4], d = x[base + (long long)W * C4 + C4];
        float4 m;
        m.x = fmaxf(fmaxf(a.x, b.x), fmaxf(cc.x, d.x));
        m.y = fmaxf(fmaxf(a.y, b.y), fmaxf(cc.y, d.y));
        m.z = fmaxf(fmaxf(a.z, b.z), fmaxf(cc.z, d.z));
        m.w = fmaxf(fmaxf(a.w, b.w), fmaxf(cc.w, d.w));
        y[i] = m;
    }
}
void launch_maxpool_fwd(const float* x, float* y, int N, int H, int W, int C, hipStream_t s)
{
    const long long total = (long long)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(cap_blocks(total, 256)), dim3(256), 0, s,
                       (const float4*)x, (float4*)y, N, H, W, C / 4);
}

// gradient to the first maximal element of the window; optional ReLU mask of
// the producing conv (x is that conv's post-ReLU output): dx *= (x > 0).
static __device__ __forceinline__ void route(float a, float b, float c, float d, float g, int relu,
                                            float& oa, float& ob, float& oc, float& od)
{
    int bi = 0; float m = a;
    if (b > m) { m = b; bi = 1; }
    if (c > m) { m = c; bi = 2; }
    if (d > m) { m = d; bi = 3; }
    if (relu && !(m > 0.f)) g = 0.f;
    oa = bi == 0 ? g : 0.f; ob = bi == 1 ? g : 0.f; oc = bi == 2 ? g : 0.f; od = bi == 3 ? g : 0.f;
}
__global__ void maxpool_bwd_kernel(const float4* x, const float4* dy, float4* dx, int N, int H, int W,
                                   int C4, int relu)
{
    const int Ho = H / 2, Wo = W / 2;
    const long long total = (long long)N * Ho * Wo * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long t = i / C4;
        const int w = (int)(t % Wo); t /= Wo;
        const int h = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const long long b0 = (((long long)n * H + 2 * h) * W + 2 * w) * C4 + c;
        const long long b1 = b0 + C4, b2 = b0 + (long long)W * C4, b3 = b2 + C4;
        const float4 a = x[b0], b = x[b1], cc = x[b2], d = x[b3], g = dy[i];
        float4 oa, ob, oc, od;
        route(a.x, b.x, cc.x, d.x, g.x, relu, oa.x, ob.x, oc.x, od.x);
        route(a.y, b.y, cc.y, d.y, g.y, relu, oa.y, ob.y, oc.y, od.y);
        route(a.z, b.z, cc.z, d.z, g.z, relu, oa.z, ob.z, oc.z, od.z);
        route(a.w, b.w, cc.w, d.w, g.w, relu, oa.w, ob.w, oc.w, od.w);
        dx[b0] = oa; dx[b1] = ob; dx[b2] = oc; dx[b3] = od;
    }
}
void launch_maxpool_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C,
                        int relu_mask, hipStream_t s)
{
    const long long total = (long long)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(cap_blocks(total, 256)), dim3(256), 0, s,
                       (const float4*)x, (const float4*)dy, (float4*)dx, N, H, W, C / 4, relu_mask);
}

// bf16_train: the same routing, but what leaves the kernel is what the block's last convolution consumes -- the interior of the zero-bordered bf16 copy
// [N][H + 2][W + 2][C] of dZ (read by its weight and data gradients) and the column sums of dZ (its bias gradient, exact fp32) -- instead of the fp32 tensor
// that a conversion pass would read back: 2.15 GB written and read again per step for block 1 at 4 x 2048x1024.  A block owns pooled rows (n, h); thread
// (c, pl) = channel quad c, pixel lane pl walks the row; the column sum of a window is its routed gradient; block partial rows, added by launch_colsum.
__global__ __launch_bounds__(256) void maxpool_bwd_bf16_kernel(const float4* __restrict__ x, const float4* __restrict__ dy, unsigned short* __restrict__ dzb,
                                                               float* __restrict__ partial, int H, int W, int C4, int lanes, int rows_per_block, int nrows, long long ps4)
{
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    __shared__ float red[256 * 4];
    const int Ho = H / 2, Wo = W / 2, Wp = W + 2, Hp = H + 2;
    const int c = threadIdx.x % C4, pl = threadIdx.x / C4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (pl < lanes) {
        for (int r = blockIdx.x * rows_per_block; r < (blockIdx.x + 1) * rows_per_block && r < nrows; ++r) {
            const int n = r / Ho, h = r - n * Ho;
            const float4* x0 = x + (((long long)n * H + 2 * h) * W) * C4;
            const float4* g0 = dy + (long long)r * Wo * C4;
            const long long q1 = ((long long)n * Hp + 2 * h + 1) * Wp + 1;                                       // padded pixel (2h + 1, 1)
            bf16x4* d0 = reinterpret_cast<bf16x4*>(dzb) + (ps4 ? (long long)(c >> 3) * ps4 + q1 * 8 + (c & 7) - c : q1 * C4);      // (d0[pix * C4 + c] below: planes step 8 per pixel)
            for (int w = pl; w < Wo; w += lanes) {
                const long long b0 = (long long)(2 * w) * C4 + c, b2 = b0 + (long long)W * C4;
                const float4 a = x0[b0], b = x0[b0 + C4], cc = x0[b2], d = x0[b2 + C4], g = g0[(long long)w * C4 + c];
                float4 oa, ob, oc, od;
                route(a.x, b.x, cc.x, d.x, g.x, 1, oa.x, ob.x, oc.x, od.x);
                route(a.y, b.y, cc.y, d.y, g.y, 1, oa.y, ob.y, oc.y, od.y);
                route(a.z, b.z, cc.z, d.z, g.z, 1, oa.z, ob.z, oc.z, od.z);
                route(a.w, b.w, cc.w, d.w, g.w, 1, oa.w, ob.w, oc.w, od.w);
                const long long pst = ps4 ? 8 : C4;                                                                 // 4-element units per pixel
                const long long p0 = (long long)(2 * w) * pst + c, p2 = p0 + (long long)Wp * pst;
                d0[p0] = bf16x4{(__bf16)oa.x, (__bf16)oa.y, (__bf16)oa.z, (__bf16)oa.w};
                d0[p0 + pst] = bf16x4{(__bf16)ob.x, (__bf16)ob.y, (__bf16)ob.z, (__bf16)ob.w};
                d0[p2] = bf16x4{(__bf16)oc.x, (__bf16)oc.y, (__bf16)oc.z, (__bf16)oc.w};
                d0[p2 + pst] = bf16x4{(__bf16)od.x, (__bf16)od.y, (__bf16)od.z, (__bf16)od.w};
                acc[0] += (oa.x + ob.x) + (oc.x + od.x); acc[1] += (oa.y + ob.y) + (oc.y + od.y);
                acc[2] += (oa.z + ob.z) + (oc.z + od.z); acc[3] += (oa.w + ob.w) + (oc.w + od.w);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[threadIdx.x * 4 + i] = acc[i];
    __syncthreads();
    if (pl == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = acc[i];
            for (int l = 1; l < lanes; ++l) v += red[(l * C4 + c) * 4 + i];
            partial[(long long)blockIdx.x * C4 * 4 + c * 4 + i] = v;
        }
    }
}
// The same from the routing bytes the forward pool kept (maxpool_fwd_route_kernel: 0..3 = the window's first maximum, 4 = not > 0): one byte per window
// instead of the four fp32 values of the block's last activation -- 4.1 GB less to read per step at 4 x 2048x1024.  Same rule, same sums: bit-identical.
__global__ __launch_bounds__(256) void maxpool_bwd_bf16_route_kernel(const unsigned* __restrict__ rt, const float4* __restrict__ dy, unsigned short* __restrict__ dzb,
                                                                     float* __restrict__ partial, int H, int W, int C4, int lanes, int rows_per_block, int nrows, long long ps4)
{
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
    __shared__ float red[256 * 8];
    const int Ho = H / 2, Wo = W / 2, Wp = W + 2, Hp = H + 2;
    const int t = threadIdx.x % C4, pl = threadIdx.x / C4;
    if (ps4) {
        // channel-chunk planes: thread t of a window = (plane p, pixel column px of the window, octet o of the plane's 32 channels) -- the eight lanes of a
        // plane write the window's two pixels of one map row as ONE contiguous 128-byte line (16 bytes each), where the quad mapping below filled half lines
        // with 8-byte stores (0.69 -> 0.78 ms when the copies became planes)
        const int p = t >> 3, px = (t >> 2) & 1, o = t & 3, c8 = p * 4 + o;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (pl < lanes) {
            for (int r = blockIdx.x * rows_per_block; r < (blockIdx.x + 1) * rows_per_block && r < nrows; ++r) {
                const int n = r / Ho, h = r - n * Ho;
                const float4* g0 = dy + (long long)r * Wo * C4;
                const unsigned* r0 = rt + (long long)r * Wo * C4;
                const long long q1 = ((long long)n * Hp + 2 * h + 1) * Wp + 1;
                bf16x8* d0 = reinterpret_cast<bf16x8*>(dzb) + (long long)p * (ps4 / 2) + o;      // (16-byte units: 4 per pixel and plane)
                for (int w = pl; w < Wo; w += lanes) {
                    const float4 ga = g0[(long long)w * C4 + 2 * c8], gb = g0[(long long)w * C4 + 2 * c8 + 1];
                    const unsigned wa = r0[(long long)w * C4 + 2 * c8], wb = r0[(long long)w * C4 + 2 * c8 + 1];
                    const float gv[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
                    bf16x8 top, bot;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const unsigned bi = ((k < 4 ? wa : wb) >> (8 * (k & 3))) & 0xffu;
                        const float vt = bi == (unsigned)px ? gv[k] : 0.f, vb = bi == (unsigned)(2 + px) ? gv[k] : 0.f;
                        top[k] = (__bf16)vt; bot[k] = (__bf16)vb;
                        acc[k] += vt + vb;
                    }
                    const long long q = q1 + 2 * w + px;
                    d0[q * 4] = top;
                    d0[(q + Wp) * 4] = bot;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) red[threadIdx.x * 8 + i] = acc[i];
        __syncthreads();
        if (pl == 0 && px == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float v = 0.f;
                for (int l = 0; l < lanes; ++l) v += red[(l * C4 + p * 8 + o) * 8 + i] + red[(l * C4 + p * 8 + 4 + o) * 8 + i];
                partial[(long long)blockIdx.x * C4 * 4 + c8 * 8 + i] = v;
            }
        }
        return;
    }
    const int c = t;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (pl < lanes) {
        for (int r = blockIdx.x * rows_per_block; r < (blockIdx.x + 1) * rows_per_block && r < nrows; ++r) {
            const int n = r / Ho, h = r - n * Ho;
            const float4* g0 = dy + (long long)r * Wo * C4;
            const unsigned* r0 = rt + (long long)r * Wo * C4;
            const long long q1 = ((long long)n * Hp + 2 * h + 1) * Wp + 1;                                       // padded pixel (2h + 1, 1)
            bf16x4* d0 = reinterpret_cast<bf16x4*>(dzb) + q1 * C4;
            for (int w = pl; w < Wo; w += lanes) {
                const float4 g = g0[(long long)w * C4 + c];
                const unsigned word = r0[(long long)w * C4 + c];
                const float gv[4] = {g.x, g.y, g.z, g.w};
                float o[4][4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned bi = (word >> (8 * k)) & 0xffu;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e][k] = bi == (unsigned)e ? gv[k] : 0.f;
                }
                const long long p0 = (long long)(2 * w) * C4 + c, p2 = p0 + (long long)Wp * C4;
                d0[p0] = bf16x4{(__bf16)o[0][0], (__bf16)o[0][1], (__bf16)o[0][2], (__bf16)o[0][3]};
                d0[p0 + C4] = bf16x4{(__bf16)o[1][0], (__bf16)o[1][1], (__bf16)o[1][2], (__bf16)o[1][3]};
                d0[p2] = bf16x4{(__bf16)o[2][0], (__bf16)o[2][1], (__bf16)o[2][2], (__bf16)o[2][3]};
                d0[p2 + C4] = bf16x4{(__bf16)o[3][0], (__bf16)o[3][1], (__bf16)o[3][2], (__bf16)o[3][3]};
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] += (o[0][k] + o[1][k]) + (o[2][k] + o[3][k]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[threadIdx.x * 4 + i] = acc[i];
    __syncthreads();
    if (pl == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = acc[i];
            for (int l = 1; l < lanes; ++l) v += red[(l * C4 + c) * 4 + i];
            partial[(long long)blockIdx.x * C4 * 4 + c * 4 + i] = v;
        }
    }
}
// dzb points at padded pixel 0 of the copy (border zero already); db[c] += column sums of dZ.  Returns false if the shape is not covered.
// x: the block's last activation, or nullptr with `route` = the forward pool's routing bytes
bool launch_maxpool_bwd_bf16(const float* x, const float* dy, unsigned short* dzb, float* db, int N, int H, int W, int C, hipStream_t s, const unsigned char* route, long long dzb_ps)
{
    const int C4 = C / 4;
    if (C % 4 || C4 > 256 || H % 2 || W % 2) return false;
    const int lanes = 256 / C4, nrows = N * (H / 2), Wo = W / 2;
    int rpb = (8 * lanes + Wo - 1) / Wo;                 // >= 8 windows per thread
    if (rpb < 1) rpb = 1;
    while ((nrows + rpb - 1) / rpb > 2048) rpb *= 2;
    const int blocks = (nrows + rpb - 1) / rpb;
    float* partial = det_scratch(s, (size_t)blocks * C);
    if (!partial) return false;
    if (route) hipLaunchKernelGGL(maxpool_bwd_bf16_route_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const unsigned*)route, (const float4*)dy, dzb, partial, H, W, C4, lanes, rpb, nrows, dzb_ps / 4);
    else hipLaunchKernelGGL(maxpool_bwd_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float4*)x, (const float4*)dy, dzb, partial, H, W, C4, lanes, rpb, nrows, dzb_ps / 4);
    if (db) launch_colsum(partial, db, blocks, C, s);
    return true;
}

// which element of each 2x2 window maxpool_bwd_kernel routes to (0..3, first maximum; 4 = the maximum is not > 0: no gradient) -- the
// record fcn8s_get_pool_routing hands to the parity checker for blocks whose routing is not already kept as argmax bytes
__global__ void maxpool_route_kernel(const float* x, unsigned char* r, int N, int H, int W, int C)
{
    const int Ho = H / 2, Wo = W / 2;
    const long long total = (long long)N * Ho * Wo * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long t = i / C;
        const int w = (int)(t % Wo); t /= Wo;
        const int h = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const long long b0 = (((long long)n * H + 2 * h) * W + 2 * w) * C + c;
        float oa, ob, oc, od;
        route(x[b0], x[b0 + C], x[b0 + (long long)W * C], x[b0 + (long long)W * C + C], 1.f, 1, oa, ob, oc, od);
        r[i] = oa != 0.f ? 0 : ob != 0.f ? 1 : oc != 0.f ? 2 : od != 0.f ? 3 : 4;
    }
}
// forward max-pool that also keeps the routing bytes (same rule, same layout as the Winograd output transform's argmax bytes): the backward
// pass of a block whose last conv did not come from that transform (the bf16 modes) can then route d(pool) inside wino_dout_kernel too
// yb16 (bf16_train): the pooled map also -- or, with y == nullptr, only -- as the interior of the consumer's zero-bordered bf16 copy [N][H/2 + 2 pad][W/2 + 2 pad][C]
// ps4: plane stride of yb16 in 4-element units (channel-chunk planes [C / 32][rows][32]), 0 = [rows][C]
// round16 (bf16_train, the pools whose output only bf16 convolutions read): the window's maximum is picked among the values ROUNDED to bf16 -- the values the
// consumers see, and the rule of maxpool_fwd_route16_kernel below, which reads the block's last activation as its bf16 copy
__global__ void maxpool_fwd_route_kernel(const float4* x, float4* y, unsigned* r, int N, int H, int W, int C4, unsigned short* yb16, int pad, long long ps4, int round16)
{
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    const int Ho = H / 2, Wo = W / 2;
    const long long total = (long long)N * Ho * Wo * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long t = i / C4;
        const int w = (int)(t % Wo); t /= Wo;
        const int h = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const long long base = (((long long)n * H + 2 * h) * W + 2 * w) * C4 + c;
        const float4 a = x[base], b = x[base + C4], cc = x[base + (long long)W * C4], d = x[base + (long long)W * C4 + C4];
        const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w}, cv[4] = {cc.x, cc.y, cc.z, cc.w}, dv[4] = {d.x, d.y, d.z, d.w};
        float mv[4]; unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float ra = round16 ? (float)(__bf16)av[k] : av[k], rbv = round16 ? (float)(__bf16)bv[k] : bv[k];
            const float rc = round16 ? (float)(__bf16)cv[k] : cv[k], rd = round16 ? (float)(__bf16)dv[k] : dv[k];
            unsigned bi = 0; float m = ra;
            if (rbv > m) { m = rbv; bi = 1; }
            if (rc > m) { m = rc; bi = 2; }
            if (rd > m) { m = rd; bi = 3; }
            if (!(m > 0.f)) bi = 4;
            mv[k] = fmaxf(fmaxf(av[k], bv[k]), fmaxf(cv[k], dv[k]));
            word |= bi << (8 * k);
        }
        if (y) y[i] = make_float4(mv[0], mv[1], mv[2], mv[3]);
        r[i] = word;
        if (yb16) {
            const long long q = ((long long)n * (Ho + 2 * pad) + h + pad) * (Wo + 2 * pad) + w + pad;
            reinterpret_cast<bf16x4*>(yb16)[ps4 ? (long long)(c >> 3) * ps4 + q * 8 + (c & 7) : q * C4 + c] = bf16x4{(__bf16)mv[0], (__bf16)mv[1], (__bf16)mv[2], (__bf16)mv[3]};
        }
    }
}
void launch_maxpool_fwd_route(const float* x, float* y, unsigned char* r, int N, int H, int W, int C, hipStream_t s, unsigned short* yb16, int pad, long long yb16_ps, int round16)
{
    const long long total = (long long)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(maxpool_fwd_route_kernel, dim3(cap_blocks(total, 256)), dim3(256), 0, s, (const float4*)x, (float4*)y, (unsigned*)r, N, H, W, C / 4, yb16, pad, yb16_ps / 4, round16);
}
// The same pool over the block's last activation kept ONLY as a bf16 copy (bf16_train: channel-chunk planes [C / 32][rows][32] of the zero-bordered map
// [N][H + 2][W + 2]): half the bytes to read, and the producing convolution wrote half the bytes.  The maximum of the bf16 values IS the bf16 rounding of the
// fp32 maximum (rounding is monotone), so the consumer's copy gets the same values; the routing bytes pick the first maximum among the bf16 values (round16 above).
__global__ void maxpool_fwd_route16_kernel(const unsigned short* __restrict__ xb, long long xps4, unsigned* r, int N, int H, int W, int C4, unsigned short* yb16, int pad, long long ps4)
{
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    const int Ho = H / 2, Wo = W / 2, Wp = W + 2, Hp = H + 2;
    const long long total = (long long)N * Ho * Wo * C4;
    const bf16x4* x4 = reinterpret_cast<const bf16x4*>(xb);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long t = i / C4;
        const int w = (int)(t % Wo); t /= Wo;
        const int h = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const long long q0 = ((long long)n * Hp + 2 * h + 1) * Wp + 2 * w + 1;                 // padded position of the window's first pixel
        const long long b0 = (long long)(c >> 3) * xps4 + q0 * 8 + (c & 7);
        const bf16x4 a = x4[b0], b = x4[b0 + 8], cc = x4[b0 + (long long)Wp * 8], d = x4[b0 + (long long)Wp * 8 + 8];
        bf16x4 mx; unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float fa = (float)a[k], fb = (float)b[k], fc = (float)cc[k], fd = (float)d[k];
            unsigned bi = 0; float m = fa;
            if (fb > m) { m = fb; bi = 1; }
            if (fc > m) { m = fc; bi = 2; }
            if (fd > m) { m = fd; bi = 3; }
            if (!(m > 0.f)) bi = 4;
            mx[k] = (__bf16)fmaxf(fmaxf(fa, fb), fmaxf(fc, fd));
            word |= bi << (8 * k);
        }
        r[i] = word;
        const long long q = ((long long)n * (Ho + 2 * pad) + h + pad) * (Wo + 2 * pad) + w + pad;
        reinterpret_cast<bf16x4*>(yb16)[(long long)(c >> 3) * ps4 + q * 8 + (c & 7)] = mx;
    }
}
void launch_maxpool_fwd_route16(const unsigned short* xb, long long xb_ps, unsigned char* r, int N, int H, int W, int C, hipStream_t s, unsigned short* yb16, int pad, long long yb16_ps)
{
    const long long total = (long long)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(maxpool_fwd_route16_kernel, dim3(cap_blocks(total, 256)), dim3(256), 0, s, xb, xb_ps / 4, (unsigned*)r, N, H, W, C / 4, yb16, pad, yb16_ps / 4);
}
void launch_maxpool_route(const float* x, unsigned char* r, int N, int H, int W, int C, hipStream_t s)
{
    const long long total = (long long)N * (H / 2) * (W / 2) * C;
    hipLaunchKernelGGL(maxpool_route_kernel, dim3(cap_blocks(total, 256)), dim3(256), 0, s, x, r, N, H, W, C);
}

// ---- block reduction helper --------------------------------------------------
static __device__ __forceinline__ double block_sum(double v, double* sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double t = 0;
    if (threadIdx.x == 0) for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
    return t;   // valid in thread 0
}

// ---- K10: fused softmax cross-entropy (loss partial sums + dlogits) ---------
// PH (XentPhase, fcn8s_internal.h) picks the loss: XENT_PLAIN is the reference's mean (the arithmetic of every default launch);
// XENT_WEIGHTED gathers the class weight w_y (LDS) into the loss and the gradient scale and counts the valid pixels; XENT_OHEM_LOSS
// writes the pixel-indexed l_p, its top-11-bit histogram and the counts |V|, |{l >= tau}| (no gradient, no loss partials);
// XENT_OHEM_GRAD keeps the pixels with l_p >= t (l_p read back from that buffer: the kept set is exactly the selected one) and scales them
// by w_y * gscale, t and gscale read from the device state the selection kernels left.
// PX (fcn8s_op_softmax_xent_px, the boundary-weighted cross-entropy; XENT_WEIGHTED and XENT_OHEM_GRAD only): the weight of pixel p is fl(w_y * tab[codes[p]]), tab = the 256 weights
// per distance code in LDS next to the class weights.  A template flag, not a branch: PX == false is the code the default phases had before.
constexpr int XENT_PIX_PER_BLOCK = 1024;
int softmax_xent_blocks(long long npix)
{
    long long b = (npix + XENT_PIX_PER_BLOCK - 1) / XENT_PIX_PER_BLOCK;
    return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}
constexpr int OHEM_BINS0 = 2048, OHEM_BINS1 = 2048, OHEM_BINS2 = 1024;     // l_p's float bits 31..21 / 20..10 / 9..0 (non-negative floats order as integers)

// the block's valid / above-tau counts and (XENT_OHEM_LOSS) its LDS histogram, folded into the model's state: integer atomics, order-independent
template <int PH>
static __device__ __forceinline__ void xent_fold(unsigned nv, unsigned ntau, unsigned* cnt, const unsigned* hsh, const XentEx& x)
{
    for (int o = 32; o > 0; o >>= 1) { nv += __shfl_down(nv, o, 64); ntau += __shfl_down(ntau, o, 64); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&cnt[0], nv); atomicAdd(&cnt[1], ntau); }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&x.st->valid, (unsigned long long)cnt[0]);
        if (PH == XENT_OHEM_LOSS) atomicAdd(&x.st->ntau, (unsigned long long)cnt[1]);
    }
    if constexpr (PH == XENT_OHEM_LOSS)
        for (int i = threadIdx.x; i < OHEM_BINS0; i += blockDim.x) if (hsh[i]) atomicAdd(&x.hist[i], hsh[i]);
}

template <int C, int PH, bool PX>   // C % 4 == 0: registers hold the pixel's logits
__global__ __launch_bounds__(256) void softmax_xent_kernel_c(const float* logits, const uint8_t* labels,
                                                             float* dlogits, double* partials,
                                                             long long npix, float gscale, float* colsum, const PixMap map, const XentEx x)
{
    // One thread = one pixel, but a pixel's C floats are C / 4 16-byte units 4 C bytes apart: read per thread, every load instruction of a
    // wave touches 64 x 16 B spread over 64 x 4C bytes (3.9 TB/s).  So a wave moves its 64 pixels as a block -- U coalesced 1 KiB
    // accesses (lane l <-> unit i * 64 + l) -- through a wave-private LDS patch from which every lane picks up its own pixel (units
    // l * U + j: stride 4C bytes = 20 banks for C = 20, conflict-free for 16-byte reads), and takes the gradient back the same way.
    constexpr int U = C / 4;
    __shared__ float4 patch[U > 1 ? 4 * 64 * U : 1];
    __shared__ double sh[4];
    __shared__ float cs[C];
    __shared__ float wsh[PH != XENT_PLAIN ? C : 1];
    __shared__ float tab[PX ? 256 : 1];
    __shared__ unsigned hsh[PH == XENT_OHEM_LOSS ? OHEM_BINS0 : 1];
    __shared__ unsigned cnt[2];
    float csum[C];                             // colsum != nullptr: column sums of dlogits (= the last bias gradient), saves a pass over dlogits
#pragma unroll
    for (int i = 0; i < C; ++i) csum[i] = 0.f;
    if (threadIdx.x < C) cs[threadIdx.x] = 0.f;
    float tsel = 0.f, gsel = gscale;           // XENT_OHEM_GRAD: the threshold t and the scale 1 / |K|
    unsigned nv = 0, ntau = 0;
    if constexpr (PH != XENT_PLAIN) {
        if (threadIdx.x < C) wsh[threadIdx.x] = x.cw[threadIdx.x];
        if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
        if constexpr (PX) for (int i = threadIdx.x; i < 256; i += blockDim.x) tab[i] = x.ptab[i];
        if constexpr (PH == XENT_OHEM_LOSS) for (int i = threadIdx.x; i < OHEM_BINS0; i += blockDim.x) hsh[i] = 0;
        if constexpr (PH == XENT_OHEM_GRAD) { tsel = x.st->t; gsel = x.st->gscale * x.ce_scale; }
        __syncthreads();
    }
    double lsum = 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4* wp = patch + (U > 1 ? wave * 64 * U : 0);
    const long long nunits = npix * U;
    for (long long p0 = blockIdx.x * (long long)blockDim.x + wave * 64; p0 < npix; p0 += (long long)gridDim.x * blockDim.x) {    // wave-uniform
        const long long p = p0 + lane;
        const long long pix = p < npix ? slot_pixel(p, map) : -1;          // npix counts slots here; labels are indexed by pixel
        float v[C];
        if constexpr (U > 1) {
            const float4* src = reinterpret_cast<const float4*>(logits) + p0 * U;
#pragma unroll
            for (int i = 0; i < U; ++i) { const int u = i * 64 + lane; if (p0 * U + u < nunits) wp[u] = src[u]; }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < U; ++i) { const float4 t = wp[lane * U + i]; v[4*i] = t.x; v[4*i+1] = t.y; v[4*i+2] = t.z; v[4*i+3] = t.w; }
            __builtin_amdgcn_wave_barrier();
        } else {
            const float4 t = p < npix ? reinterpret_cast<const float4*>(logits)[p] : make_float4(0.f, 0.f, 0.f, 0.f);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        }
        float4 g[U];
#pragma unroll
        for (int i = 0; i < U; ++i) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);       // a slot outside the image: its gradient is defined as 0
        if (pix >= 0) {
            float m = v[0];
#pragma unroll
            for (int i = 1; i < C; ++i) m = fmaxf(m, v[i]);
            float e[C]; float s = 0.f;
#pragma unroll
            for (int i = 0; i < C; ++i) { e[i] = expf(v[i] - m); s += e[i]; }
            const int lab = labels[pix];
            const bool ign = lab >= C;                 // ids outside [0, C) (e.g. a 255 "ignore" id, an all-zero one-hot row): no loss, no gradient
            float vl = 0.f;
#pragma unroll
            for (int i = 0; i < C; ++i) vl = (i == lab) ? v[i] : vl;
            float gs = gscale;                          // this pixel's gradient scale
            bool keep = !ign;
            if constexpr (PH == XENT_PLAIN) {
                if (!ign) lsum += (double)(m + logf(s) - vl);
            } else if constexpr (PH == XENT_WEIGHTED) {
                float w = ign ? 0.f : wsh[lab];
                if constexpr (PX) w *= tab[x.codes[pix]];
                gs = gscale * w; nv += !ign;
                if (!ign) lsum += (double)w * (double)(m + logf(s) - vl);
            } else if constexpr (PH == XENT_OHEM_LOSS) {
                const float l = m + logf(s) - vl;          // >= 0: fl(m + log s) >= m >= v[lab]
                if (!ign) { ++nv; ntau += l >= x.tau; atomicAdd(&hsh[__float_as_uint(l) >> 21], 1u); }
                x.lbuf[pix] = ign ? -1.f : l;
            } else {
                const float l = x.lbuf[pix];               // -1 for an ignored pixel: never kept (t >= 0)
                keep = !ign && l >= tsel;
                float w = keep ? wsh[lab] : 0.f;
                if constexpr (PX) w *= tab[x.codes[pix]];
                gs = gsel * w;
                if (keep) lsum += (double)w * (double)l;
            }
            if (PH != XENT_OHEM_LOSS && dlogits) {
                const float inv = keep ? gs / s : 0.f;
#pragma unroll
                for (int i = 0; i < U; ++i) {
                    float4 t;
                    t.x = e[4*i] * inv - ((4*i) == lab ? gs : 0.f);
                    t.y = e[4*i+1] * inv - ((4*i+1) == lab ? gs : 0.f);
                    t.z = e[4*i+2] * inv - ((4*i+2) == lab ? gs : 0.f);
                    t.w = e[4*i+3] * inv - ((4*i+3) == lab ? gs : 0.f);
                    g[i] = t;
                    csum[4*i] += t.x; csum[4*i+1] += t.y; csum[4*i+2] += t.z; csum[4*i+3] += t.w;
                }
            }
        }
        if (PH != XENT_OHEM_LOSS && dlogits) {
            if constexpr (U > 1) {
#pragma unroll
                for (int i = 0; i < U; ++i) wp[lane * U + i] = g[i];
                __builtin_amdgcn_wave_barrier();
                float4* dst = reinterpret_cast<float4*>(dlogits) + p0 * U;
#pragma unroll
                for (int i = 0; i < U; ++i) { const int u = i * 64 + lane; if (p0 * U + u < nunits) dst[u] = wp[u]; }
                __builtin_amdgcn_wave_barrier();
            } else if (p < npix) reinterpret_cast<float4*>(dlogits)[p] = g[0];
        }
    }
    if constexpr (PH == XENT_WEIGHTED || PH == XENT_OHEM_LOSS) xent_fold<PH>(nv, ntau, cnt, hsh, x);
    if constexpr (PH == XENT_OHEM_LOSS) return;
    const double t = block_sum(lsum, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
    if (colsum && dlogits) {
#pragma unroll
        for (int i = 0; i < C; ++i) {
            float v = csum[i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if ((threadIdx.x & 63) == 0) atomicAdd(&cs[i], v);
        }
        __syncthreads();
        if (threadIdx.x < C) unsafeAtomicAdd(colsum + threadIdx.x, cs[threadIdx.x]);
    }
}
template <int PH, bool PX>
__global__ __launch_bounds__(256) void softmax_xent_kernel_any(const float* logits, const uint8_t* labels,
                                                               float* dlogits, double* partials,
                                                               long long npix, int C, float gscale, const PixMap map, const XentEx x)
{
    __shared__ double sh[4];
    __shared__ float wsh[PH != XENT_PLAIN ? 64 : 1];
    __shared__ float tab[PX ? 256 : 1];
    __shared__ unsigned hsh[PH == XENT_OHEM_LOSS ? OHEM_BINS0 : 1];
    __shared__ unsigned cnt[2];
    float tsel = 0.f, gsel = gscale;
    unsigned nv = 0, ntau = 0;
    if constexpr (PH != XENT_PLAIN) {
        if (threadIdx.x < C) wsh[threadIdx.x] = x.cw[threadIdx.x];
        if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
        if constexpr (PX) for (int i = threadIdx.x; i < 256; i += blockDim.x) tab[i] = x.ptab[i];
        if constexpr (PH == XENT_OHEM_LOSS) for (int i = threadIdx.x; i < OHEM_BINS0; i += blockDim.x) hsh[i] = 0;
        if constexpr (PH == XENT_OHEM_GRAD) { tsel = x.st->t; gsel = x.st->gscale * x.ce_scale; }
        __syncthreads();
    }
    double lsum = 0;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix;
         p += (long long)gridDim.x * blockDim.x) {
        const long long pix = slot_pixel(p, map);
        if (pix < 0) { if (PH != XENT_OHEM_LOSS && dlogits) for (int i = 0; i < C; ++i) dlogits[p * C + i] = 0.f; continue; }
        const float* l = logits + p * C;
        float m = l[0];
        for (int i = 1; i < C; ++i) m = fmaxf(m, l[i]);
        float s = 0.f;
        for (int i = 0; i < C; ++i) s += expf(l[i] - m);
        const int lab = labels[pix];
        const bool ign = lab >= C;                 // see softmax_xent_kernel_c
        float gs = gscale;
        bool keep = !ign;
        if constexpr (PH == XENT_PLAIN) {
            if (!ign) lsum += (double)(m + logf(s) - l[lab]);
        } else if constexpr (PH == XENT_WEIGHTED) {
            float w = ign ? 0.f : wsh[lab];
            if constexpr (PX) w *= tab[x.codes[pix]];
            gs = gscale * w; nv += !ign;
            if (!ign) lsum += (double)w * (double)(m + logf(s) - l[lab]);
        } else if constexpr (PH == XENT_OHEM_LOSS) {
            const float lp = ign ? -1.f : m + logf(s) - l[lab];
            if (!ign) { ++nv; ntau += lp >= x.tau; atomicAdd(&hsh[__float_as_uint(lp) >> 21], 1u); }
            x.lbuf[pix] = lp;
            continue;
        } else {
            const float lp = x.lbuf[pix];
            keep = !ign && lp >= tsel;
            float w = keep ? wsh[lab] : 0.f;
            if constexpr (PX) w *= tab[x.codes[pix]];
            gs = gsel * w;
            if (keep) lsum += (double)w * (double)lp;
        }
        if (dlogits) {
            const float inv = keep ? gs / s : 0.f;
            for (int i = 0; i < C; ++i) dlogits[p * C + i] = expf(l[i] - m) * inv - (i == lab ? gs : 0.f);
        }
    }
    if constexpr (PH == XENT_WEIGHTED || PH == XENT_OHEM_LOSS) xent_fold<PH>(nv, ntau, cnt, hsh, x);
    if constexpr (PH == XENT_OHEM_LOSS) return;
    const double t = block_sum(lsum, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
template <int PH, bool PX = false>
static void xent_launch(const float* logits, const uint8_t* labels, float* dlogits, double* partials, long long npix, long long nslot, int C,
                        float gscale, float* colsum, const PixMap& pm, const XentEx& x, hipStream_t s)
{
    const int blocks = softmax_xent_blocks(npix);          // (the partial-sum count finalize_loss expects)
    // the fused column sums (= the last bias gradient) of the blocks meet in atomics: deterministic mode takes them from dlogits in a pass of its own
    // (slots outside the image hold zero gradient); so does the generic kernel
    const bool fused = colsum && dlogits && (C == 20 || C == 4) && !t_deterministic;
    float* cs = fused ? colsum : nullptr;
    if (C == 20)     hipLaunchKernelGGL((softmax_xent_kernel_c<20, PH, PX>), dim3(blocks), dim3(256), 0, s, logits, labels, dlogits, partials, nslot, gscale, cs, pm, x);
    else if (C == 4) hipLaunchKernelGGL((softmax_xent_kernel_c<4, PH, PX>), dim3(blocks), dim3(256), 0, s, logits, labels, dlogits, partials, nslot, gscale, cs, pm, x);
    else             hipLaunchKernelGGL((softmax_xent_kernel_any<PH, PX>), dim3(blocks), dim3(256), 0, s, logits, labels, dlogits, partials, nslot, C, gscale, pm, x);
    if (colsum && dlogits && !fused) launch_colsum(dlogits, colsum, nslot, C, s);
}
void launch_softmax_xent(const float* logits, const uint8_t* labels, float* dlogits, double* partials,
                         long long npix, int C, float grad_scale, hipStream_t s, float* colsum, const PixMap* map, int N)
{
    const PixMap pm = map ? *map : PixMap{0, 0, 0, 0, 0, 0};
    xent_launch<XENT_PLAIN>(logits, labels, dlogits, partials, npix, pixmap_slots(pm, npix, N), C, grad_scale, colsum, pm, XentEx{}, s);
}

// ---- OHEM: the k-th largest l_p by radix selection, all on the device ----------------------------------------------------------------
// Level 1 / 2 histogram bits 20..10 / 9..0 of the keys (= l_p's float bits, valid pixels only) whose higher bits equal the prefix fixed so
// far; a level whose selection is already settled (st->active == 0) returns at once.
__global__ __launch_bounds__(256) void ohem_refine_kernel(const float* __restrict__ lbuf, long long npix, const OhemState* st, unsigned* hist, int level)
{
    if (!st->active) return;
    __shared__ unsigned h[OHEM_BINS1];
    const int hi = level == 1 ? 21 : 10, shift = level == 1 ? 10 : 0;
    const unsigned mask = level == 1 ? OHEM_BINS1 - 1 : OHEM_BINS2 - 1, want = st->prefix >> hi;
    for (int i = threadIdx.x; i < OHEM_BINS1; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const unsigned key = __float_as_uint(lbuf[p]);
        if ((int)key >= 0 && (key >> hi) == want) atomicAdd(&h[(key >> shift) & mask], 1u);    // (an ignored pixel holds -1: sign bit set)
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= (int)mask; i += blockDim.x) if (h[i]) atomicAdd(&hist[i], h[i]);
}
// One block.  Level 0 decides whether the selection is needed at all: k = min(min_kept, |V|); with k == 0 or |{l >= tau}| >= k the
// k-th largest is >= tau, so t = tau and |K| = |{l >= tau}|.  Otherwise every level finds the bin that holds the k-th largest of the keys
// under the prefix (chunk sums, a suffix scan over the 256 chunks, one thread walks the crossing chunk), and the last level fixes
// t = l_(k) < tau and |K| = |{l >= l_(k)}| = (keys above the bin at every level) + (the bin's count).
__global__ __launch_bounds__(256) void ohem_select_kernel(OhemState* st, const unsigned* hist, int level, long long min_kept, float tau)
{
    __shared__ unsigned long long part[256];
    __shared__ unsigned long long krem, above0;
    __shared__ int act;
    const int t = threadIdx.x;
    if (t == 0) {
        if (level == 0) {
            const unsigned long long V = st->valid, k = (unsigned long long)min_kept < V ? (unsigned long long)min_kept : V;
            if (k == 0 || st->ntau >= k) {
                st->active = 0; st->t = tau; st->kept = st->ntau; st->gscale = st->ntau ? 1.f / (float)st->ntau : 0.f;
            } else { st->active = 1; st->krem = k; st->above = 0; st->prefix = 0; }
        }
        act = st->active; krem = st->krem; above0 = st->above;
    }
    __syncthreads();
    if (!act) return;
    const int nb = level == 2 ? OHEM_BINS2 : OHEM_BINS0, per = nb / 256, shift = level == 0 ? 21 : level == 1 ? 10 : 0;
    unsigned long long c = 0;
    for (int j = 0; j < per; ++j) c += hist[t * per + j];
    part[t] = c;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {           // part[t] = sum of chunks t .. 255
        const unsigned long long v = part[t] + (t + off < 256 ? part[t + off] : 0ull);
        __syncthreads();
        part[t] = v;
        __syncthreads();
    }
    const unsigned long long incl = part[t], excl = t < 255 ? part[t + 1] : 0ull;
    if (excl < krem && incl >= krem) {                   // exactly one chunk holds the k-th largest (krem >= 1, <= the keys under the prefix)
        unsigned long long above = excl;
        int bin = t * per;
        unsigned h = 0;
        for (int j = per - 1; j >= 0; --j) { h = hist[t * per + j]; if (above + h >= krem) { bin = t * per + j; break; } above += h; }
        const unsigned prefix = st->prefix | ((unsigned)bin << shift);
        st->prefix = prefix; st->krem = krem - above; st->above = above0 + above;
        if (level == 2) {
            const unsigned long long kept = above0 + above + h;
            st->t = __uint_as_float(prefix); st->kept = kept; st->gscale = 1.f / (float)kept;
        }
    }
}
void launch_softmax_xent_ex(const float* logits, const uint8_t* labels, float* dlogits, double* partials, long long npix, int C, float grad_scale,
                            hipStream_t s, float* colsum, const PixMap* map, int N, const XentEx& x, float ohem_thresh, long long ohem_min_kept)
{
    const PixMap pm = map ? *map : PixMap{0, 0, 0, 0, 0, 0};
    const long long nslot = pixmap_slots(pm, npix, N);
    hipMemsetAsync(x.st, 0, LOSS_SCRATCH_BYTES, s);                 // the state and the three histograms (x.hist follows x.st)
    const bool px = x.codes && x.ptab;                              // fcn8s_op_softmax_xent_px: per-pixel weights by distance code
    if (ohem_thresh <= 0.f) {
        if (px) xent_launch<XENT_WEIGHTED, true>(logits, labels, dlogits, partials, npix, nslot, C, grad_scale, colsum, pm, x, s);
        else    xent_launch<XENT_WEIGHTED>(logits, labels, dlogits, partials, npix, nslot, C, grad_scale, colsum, pm, x, s);
        return;
    }
    XentEx y = x;
    y.tau = (float)(-log((double)ohem_thresh));
    xent_launch<XENT_OHEM_LOSS>(logits, labels, nullptr, partials, npix, nslot, C, grad_scale, nullptr, pm, y, s);
    const int rb = cap_blocks(npix, 1024);
    hipLaunchKernelGGL(ohem_select_kernel, dim3(1), dim3(256), 0, s, x.st, x.hist, 0, ohem_min_kept, y.tau);
    hipLaunchKernelGGL(ohem_refine_kernel, dim3(rb), dim3(256), 0, s, (const float*)x.lbuf, npix, (const OhemState*)x.st, x.hist + OHEM_BINS0, 1);
    hipLaunchKernelGGL(ohem_select_kernel, dim3(1), dim3(256), 0, s, x.st, x.hist + OHEM_BINS0, 1, ohem_min_kept, y.tau);
    hipLaunchKernelGGL(ohem_refine_kernel, dim3(rb), dim3(256), 0, s, (const float*)x.lbuf, npix, (const OhemState*)x.st, x.hist + OHEM_BINS0 + OHEM_BINS1, 2);
    hipLaunchKernelGGL(ohem_select_kernel, dim3(1), dim3(256), 0, s, x.st, x.hist + OHEM_BINS0 + OHEM_BINS1, 2, ohem_min_kept, y.tau);
    if (px) xent_launch<XENT_OHEM_GRAD, true>(logits, labels, dlogits, partials, npix, nslot, C, grad_scale, colsum, pm, y, s);
    else    xent_launch<XENT_OHEM_GRAD>(logits, labels, dlogits, partials, npix, nslot, C, grad_scale, colsum, pm, y, s);
}

__global__ void finalize_loss_kernel(const double* partials, int nparts, long long npix, const float* regsum,
                                     float rate, float* loss_out, const unsigned long long* den, float* terms)
{
    __shared__ double sh[4];
    double v = 0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) v += partials[i];
    const double t = block_sum(v, sh);
    if (threadIdx.x == 0) {
        const float ce = den ? (*den ? (float)(t / (double)*den) : 0.f) : (float)(t / (double)npix);
        const float reg = regsum ? 0.5f * rate * regsum[0] : 0.f;
        loss_out[0] = ce + reg;
        if (terms) { terms[0] = ce; terms[1] = 0.f; terms[2] = reg; }
    }
}
void launch_finalize_loss(const double* partials, int nparts, long long npix, const float* regsum,
                          float rate, float* loss_out, hipStream_t s, const unsigned long long* den, float* terms)
{
    hipLaunchKernelGGL(finalize_loss_kernel, dim3(1), dim3(256), 0, s, partials, nparts, npix, regsum, rate, loss_out, den, terms);
}

// ---- K13: softmax -> argmax (of the softmax output, lowest index on ties) ----
__global__ __launch_bounds__(256) void softmax_argmax_kernel(const float* logits, float* sm, long long* am,
                                                             long long npix, int C, const PixMap map)
{
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix;
         p += (long long)gridDim.x * blockDim.x) {
        const long long pix = slot_pixel(p, map);          // outputs are always NHWC / per pixel
        if (pix < 0) continue;
        const float* l = logits + p * C;
        float m = l[0];
        for (int i = 1; i < C; ++i) m = fmaxf(m, l[i]);
        float s = 0.f;
        for (int i = 0; i < C; ++i) s += expf(l[i] - m);
        int best = 0; float bv = -1.f;
        for (int i = 0; i < C; ++i) {
            const float v = expf(l[i] - m) / s;
            if (sm) sm[pix * C + i] = v;
            if (v > bv) { bv = v; best = i; }
        }
        if (am) am[pix] = best;
    }
}
// C % 4 == 0 in registers: 16-byte loads / stores, one expf per class (same values as the generic kernel: v_i = expf(l_i - max) / sum)
template <int C>
__global__ __launch_bounds__(256) void softmax_argmax_kernel_c(const float* __restrict__ logits, float* __restrict__ sm, long long* __restrict__ am,
                                                               long long npix, const PixMap map)
{
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const long long pix = slot_pixel(p, map);
        if (pix < 0) continue;
        float v[C];
        const float4* src = reinterpret_cast<const float4*>(logits + p * C);
#pragma unroll
        for (int i = 0; i < C / 4; ++i) { const float4 t = src[i]; v[4*i] = t.x; v[4*i+1] = t.y; v[4*i+2] = t.z; v[4*i+3] = t.w; }
        float m = v[0];
#pragma unroll
        for (int i = 1; i < C; ++i) m = fmaxf(m, v[i]);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < C; ++i) { v[i] = expf(v[i] - m); s += v[i]; }
        int best = 0; float bv = -1.f;
#pragma unroll
        for (int i = 0; i < C; ++i) { v[i] = v[i] / s; if (v[i] > bv) { bv = v[i]; best = i; } }
        if (sm) {
            float4* dst = reinterpret_cast<float4*>(sm + pix * C);
#pragma unroll
            for (int i = 0; i < C / 4; ++i) dst[i] = make_float4(v[4*i], v[4*i+1], v[4*i+2], v[4*i+3]);
        }
        if (am) am[pix] = best;
    }
}
void launch_softmax_argmax(const float* logits, float* softmax_out, long long* argmax_out,
                           long long npix, int C, hipStream_t s, const PixMap* map, int N)
{
    const PixMap pm = map ? *map : PixMap{0, 0, 0, 0, 0, 0};
    const long long nslot = pixmap_slots(pm, npix, N);
    const int blocks = cap_blocks(nslot, 256);
    if (C == 20) hipLaunchKernelGGL(softmax_argmax_kernel_c<20>, dim3(blocks), dim3(256), 0, s, logits, softmax_out, argmax_out, nslot, pm);
    else if (C == 4) hipLaunchKernelGGL(softmax_argmax_kernel_c<4>, dim3(blocks), dim3(256), 0, s, logits, softmax_out, argmax_out, nslot, pm);
    else hipLaunchKernelGGL(softmax_argmax_kernel, dim3(blocks), dim3(256), 0, s, logits, softmax_out, argmax_out, nslot, C, pm);
}

// ---- the k = 2s transposed conv as one GEMM: re-layouts (PixMap in fcn8s_internal.h) --------------------------------------------
// Output pixel oy = s q - s/2 + r receives input row i = q (filter row ky = r) and i = q - 1 (ky = r + s): with rows = output
// blocks (n, q, qx), K = (a, b, ci) over the 2 x 2 input cells (q-1+a, qx-1+b) and columns = (r, rx, co), the whole layer is
// Y[rows][s*s*C] = A[rows][4C] * B2[4C][s*s*C] with B2[(a,b,ci)][(r,rx,co)] = w[r + s(1-a)][rx + s(1-b)][co][ci] -- no sub-pixel
// phases, no 20-of-32 column waste, and its two gradients are plain GEMMs over the same rows.
__global__ void tconv_im2col_kernel(const float4* __restrict__ x, float4* __restrict__ A, int N, int Hi, int Wi, int C4, int KP4)
{
    const int QH = Hi + 1, QW = Wi + 1;
    const long long total = (long long)N * QH * QW * KP4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % KP4); const long long row = i / KP4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < 4 * C4) {
            const int t = c / C4, c4 = c - t * C4, a = t >> 1, b = t & 1;
            const int qx = (int)(row % QW); const long long r2 = row / QW;
            const int q = (int)(r2 % QH); const long long n = r2 / QH;
            const int iy = q - 1 + a, ix = qx - 1 + b;
            if ((unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi) v = x[((n * Hi + iy) * Wi + ix) * C4 + c4];
        }
        A[i] = v;
    }
}
void launch_tconv_im2col(const float* x, float* A, int N, int Hi, int Wi, int C, int KP, hipStream_t s)
{
    hipLaunchKernelGGL(tconv_im2col_kernel, dim3(cap_blocks((long long)N * (Hi + 1) * (Wi + 1) * (KP / 4), 256)), dim3(256), 0, s,
                       (const float4*)x, (float4*)A, N, Hi, Wi, C / 4, KP / 4);
}
__global__ void tconv_col2im_kernel(const float4* __restrict__ dA, float4* __restrict__ dx, int N, int Hi, int Wi, int C4, int KP4)
{
    const int QH = Hi + 1, QW = Wi + 1;
    const long long total = (long long)N * Hi * Wi * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4); long long t = i / C4;
        const int ix = (int)(t % Wi); t /= Wi;
        const int iy = (int)(t % Hi); const long long n = t / Hi;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const long long row = (n * QH + (iy + 1 - a)) * QW + (ix + 1 - b);       // always inside the (Hi+1) x (Wi+1) grid
                const float4 v = dA[row * KP4 + (a * 2 + b) * C4 + c4];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
        dx[i] = acc;
    }
}
void launch_tconv_col2im(const float* dA, float* dx, int N, int Hi, int Wi, int C, int KP, hipStream_t s)
{
    hipLaunchKernelGGL(tconv_col2im_kernel, dim3(cap_blocks((long long)N * Hi * Wi * (C / 4), 256)), dim3(256), 0, s,
                       (const float4*)dA, (float4*)dx, N, Hi, Wi, C / 4, KP / 4);
}
__global__ void tconv_pack_gemm_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ b2, float* __restrict__ b2t,
                                       float* __restrict__ bias_tiled, int C, int S, int KP)
{
    const int K = 2 * S, NC = S * S * C, K4 = 4 * C;
    const long long total = (long long)NC * KP;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % KP), col = (int)(i / KP);          // b2t[col][k]
        float v = 0.f;
        if (k < K4) {
            const int t = k / C, ci = k - t * C, a = t >> 1, b = t & 1;
            const int co = col % C, rr = col / C, rx = rr % S, r = rr / S;
            const int ky = r + S * (1 - a), kx = rx + S * (1 - b);
            v = w[((long long)(ky * K + kx) * C + co) * C + ci];
            b2[(long long)k * NC + col] = v;
        }
        b2t[i] = v;
        if (k == 0) bias_tiled[col] = bias ? bias[col % C] : 0.f;
    }
}
void launch_tconv_pack_gemm(const float* w, const float* bias, float* b2, float* b2t, float* bias_tiled, int C, int S, int KP, hipStream_t s)
{
    hipLaunchKernelGGL(tconv_pack_gemm_kernel, dim3(cap_blocks((long long)S * S * C * KP, 256)), dim3(256), 0, s, w, bias, b2, b2t, bias_tiled, C, S, KP);
}
__global__ void tconv_unpack_dw_kernel(const float* __restrict__ db2, float* __restrict__ dw, int C, int S)
{
    const int K = 2 * S, NC = S * S * C;
    const long long total = (long long)K * K * C * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ci = (int)(i % C); long long t = i / C;
        const int co = (int)(t % C); t /= C;
        const int kx = (int)(t % K), ky = (int)(t / K);
        const int a = ky >= S ? 0 : 1, b = kx >= S ? 0 : 1;             // ky = r + S(1 - a)
        const int r = ky - S * (1 - a), rx = kx - S * (1 - b);
        dw[i] += db2[(long long)((a * 2 + b) * C + ci) * NC + (r * S + rx) * C + co];
    }
}
void launch_tconv_unpack_dw(const float* db2, float* dw, int C, int S, hipStream_t s)
{
    hipLaunchKernelGGL(tconv_unpack_dw_kernel, dim3(cap_blocks(4LL * S * S * C * C, 256)), dim3(256), 0, s, db2, dw, C, S);
}
__global__ void unblock_logits_kernel(const float* __restrict__ blocked, float* __restrict__ nhwc, const PixMap map, long long nslot, int C)
{
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < nslot; p += (long long)gridDim.x * blockDim.x) {
        const long long pix = slot_pixel(p, map);
        if (pix < 0) continue;
        for (int c = 0; c < C; ++c) nhwc[pix * C + c] = blocked[p * C + c];
    }
}
void launch_unblock_logits(const float* blocked, float* nhwc, const PixMap& map, int N, int C, hipStream_t s)
{
    const long long nslot = pixmap_slots(map, 0, N);
    hipLaunchKernelGGL(unblock_logits_kernel, dim3(cap_blocks(nslot, 256)), dim3(256), 0, s, blocked, nhwc, map, nslot, C);
}

// ---- one-hot rows -> uint8 class ids (first non-zero entry; counts rows that are not one-hot) ------------
template <typename T>
__global__ __launch_bounds__(256) void onehot_to_ids_kernel(const T* oh, long long npix, int C, uint8_t* ids, int* bad)
{
    int nbad = 0;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const T* row = oh + p * C;
        int first = -1, cnt = 0;
        for (int c = 0; c < C; ++c) if (row[c] != 0) { if (first < 0) first = c; ++cnt; }
        ids[p] = (uint8_t)(first < 0 ? 255 : first);      // all-zero row: the 'ignore' id (zero loss and gradient in the loss kernel)
        nbad += cnt != 1;
    }
    if (bad && nbad) atomicAdd(bad, nbad);
}
void launch_onehot_to_ids(const void* oh, int elem_bytes, long long npix, int C, uint8_t* ids, int* bad, hipStream_t s)
{
    const int blocks = cap_blocks(npix, 256);
    if (elem_bytes == 1) hipLaunchKernelGGL(onehot_to_ids_kernel<uint8_t>, dim3(blocks), dim3(256), 0, s, (const uint8_t*)oh, npix, C, ids, bad);
    else                 hipLaunchKernelGGL(onehot_to_ids_kernel<uint32_t>, dim3(blocks), dim3(256), 0, s, (const uint32_t*)oh, npix, C, ids, bad);
}

// ---- K14: confusion matrix conf[label*C + pred] += 1 --------------------------
__global__ __launch_bounds__(256) void confusion_kernel(const uint8_t* labels, const long long* pred,
                                                        long long npix, unsigned long long* conf, int C)
{
    extern __shared__ unsigned int hist[];
    const int bins = C * C;
    for (int i = threadIdx.x; i < bins; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix;
         p += (long long)gridDim.x * blockDim.x) {
        const int l = labels[p]; const int q = (int)pred[p];
        if (l < C && q >= 0 && q < C) atomicAdd(&hist[l * C + q], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += blockDim.x)
        if (hist[i]) atomicAdd(&conf[i], (unsigned long long)hist[i]);
}
void launch_confusion(const uint8_t* labels, const long long* pred, long long npix,
                      unsigned long long* conf, int C, hipStream_t s)
{
    int blocks = cap_blocks(npix, 256 * 16);
    if (blocks > 512) blocks = 512;
    hipLaunchKernelGGL(confusion_kernel, dim3(blocks), dim3(256), C * C * sizeof(unsigned int), s,
                       labels, pred, npix, conf, C);
}

// ---- column sums (bias gradients): out[c] += sum_r x[r, c] --------------------
// 16-byte loads, four independent rows in flight per thread; a block covers `rpb` rows x up to 1024 columns and reduces its
// row groups through LDS.  Blocks do NOT meet in atomics: device-scope atomics on one cache line (and equally a ticket counter
// with a fence) serialise at ~100 ns per block, so the one-kernel versions took time proportional to their block count (919
// blocks on a 60 MB slab: 125 us = 0.5 TB/s).  Each block stores its partial row; a second, one-block-per-column-tile kernel
// adds the rows up in block order (reproducible) and does the single read-modify-write of `out`.  A launch that fits one
// block per column tile writes `out` directly.
__global__ __launch_bounds__(256) void colsum_kernel(const float4* __restrict__ x, float* __restrict__ out, long long rows, int C4, int tpr,
                                                     long long rpb, float4* __restrict__ partial)
{
    __shared__ float4 sh[256];
    const int rgroups = 256 / tpr;
    const int lc = threadIdx.x % tpr, rg = threadIdx.x / tpr;
    const int c = blockIdx.y * tpr + lc;
    const long long r0 = blockIdx.x * rpb, r1 = (r0 + rpb < rows) ? r0 + rpb : rows;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C4 && rg < rgroups) {
        long long r = r0 + rg;
        for (; r + 3LL * rgroups < r1; r += 4LL * rgroups) {
            const float4 a = x[r * C4 + c], b = x[(r + rgroups) * C4 + c], d = x[(r + 2LL * rgroups) * C4 + c], e = x[(r + 3LL * rgroups) * C4 + c];
            acc.x += (a.x + b.x) + (d.x + e.x); acc.y += (a.y + b.y) + (d.y + e.y);
            acc.z += (a.z + b.z) + (d.z + e.z); acc.w += (a.w + b.w) + (d.w + e.w);
        }
        for (; r < r1; r += rgroups) { const float4 a = x[r * C4 + c]; acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w; }
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (rg == 0 && c < C4) {
        for (int g = 1; g < rgroups; ++g) { const float4 t = sh[g * tpr + lc]; acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w; }
        if (partial) partial[(long long)blockIdx.x * C4 + c] = acc;
        else { float* o = out + 4 * c; o[0] += acc.x; o[1] += acc.y; o[2] += acc.z; o[3] += acc.w; }
    }
}
// 16 float4 columns x 16 row groups per block, eight independent loads in flight per thread (the rows are L2-resident)
__global__ __launch_bounds__(256) void colsum_final_kernel(const float4* __restrict__ partial, float* __restrict__ out, int nrows, int C4)
{
    __shared__ float4 sh[256];
    const int lc = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + lc;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C4) {
        int b = rg;
        for (; b + 7 * 16 < nrows; b += 8 * 16) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[(long long)(b + 16 * u) * C4 + c];
#pragma unroll
            for (int u = 0; u < 8; ++u) { t.x += v[u].x; t.y += v[u].y; t.z += v[u].z; t.w += v[u].w; }
        }
        for (; b < nrows; b += 16) { const float4 v = partial[(long long)b * C4 + c]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
    }
    sh[threadIdx.x] = t;
    __syncthreads();
    if (rg == 0 && c < C4) {
        for (int g = 1; g < 16; ++g) { const float4 v = sh[g * 16 + lc]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
        float* o = out + 4 * c;
        o[0] += t.x; o[1] += t.y; o[2] += t.z; o[3] += t.w;
    }
}
void launch_colsum(const float* x, float* out, long long rows, int C, hipStream_t s)   // C % 4 == 0 (all channel counts here are)
{
    const int C4 = C / 4;
    int tpr = 1; while (tpr < C4 && tpr < 256) tpr *= 2;          // threads per row slice (power of two >= C4, at most 256)
    const int ctiles = (C4 + tpr - 1) / tpr, rgroups = 256 / tpr;
    long long rblocks = (rows + 16LL * rgroups - 1) / (16LL * rgroups);      // >= 16 rows per thread
    constexpr int maxb_total = 512;
    const long long maxb = maxb_total / ctiles > 0 ? maxb_total / ctiles : 1;
    if (rblocks > maxb) rblocks = maxb;
    if (rblocks < 1) rblocks = 1;
    const long long rpb = (rows + rblocks - 1) / rblocks;
    const unsigned gx = (unsigned)((rows + rpb - 1) / rpb);
    float4* partial = nullptr;
    if (gx > 1) {
        partial = (float4*)scratch2(s, (size_t)gx * C);
        if (!partial) { defer_error(FCN8S_ERR_OOM, "the column sums' scratch (%zu floats) cannot be allocated", (size_t)gx * C); return; }
    }
    hipLaunchKernelGGL(colsum_kernel, dim3(gx, ctiles), dim3(256), 0, s, (const float4*)x, out, rows, C4, tpr, rpb, partial);
    if (gx > 1) hipLaunchKernelGGL(colsum_final_kernel, dim3((C4 + 15) / 16), dim3(256), 0, s, (const float4*)partial, out, (int)gx, C4);
}

__global__ __launch_bounds__(256) void sumsq_kernel(const float* x, float* out, long long n)
{
    __shared__ double sh[4];
    double v = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        v += (double)x[i] * x[i];
    const double t = block_sum(v, sh);
    if (threadIdx.x == 0) unsafeAtomicAdd(out, (float)t);
}
void launch_sumsq(const float* x, float* out, long long n, hipStream_t s)
{
    hipLaunchKernelGGL(sumsq_kernel, dim3(t_deterministic ? 1 : cap_blocks(n, 1024)), dim3(256), 0, s, x, out, n);      // (one block: no atomics between blocks)
}

__global__ void axpy_kernel(float* y, const float* x, float a, long long n)
{
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        y[i] += a * x[i];
}
void launch_axpy(float* y, const float* x, float a, long long n, hipStream_t s)
{
    hipLaunchKernelGGL(axpy_kernel, dim3(cap_blocks(n, 256)), dim3(256), 0, s, y, x, a, n);
}

// ---- weight re-layouts ---------------------------------------------------------
// wt[T-1-t][co][ci] = w[t][ci][co]   (data-gradient weights of a SAME conv)
__global__ void flip_transpose_kernel(const float* w, float* wt, int taps, int Cin, int Cout)
{
    __shared__ float tile[32][33];
    const int t = blockIdx.z;
    const int ci0 = blockIdx.y * 32, co0 = blockIdx.x * 32;
    const float* src = w + (long long)t * Cin * Cout;
    float* dst = wt + (long long)(taps - 1 - t) * Cin * Cout;
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int ci = ci0 + r, co = co0 + threadIdx.x;
        tile[r][threadIdx.x] = (ci < Cin && co < Cout) ? src[(long long)ci * Cout + co] : 0.f;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int co = co0 + r, ci = ci0 + threadIdx.x;
        if (co < Cout && ci < Cin) dst[(long long)co * Cin + ci] = tile[threadIdx.x][r];
    }
}
void launch_flip_transpose(const float* w, float* wt, int taps, int Cin, int Cout, hipStream_t s)
{
    dim3 grid((Cout + 31) / 32, (Cin + 31) / 32, taps);
    hipLaunchKernelGGL(flip_transpose_kernel, grid, dim3(32, 8), 0, s, w, wt, taps, Cin, Cout);
}
// w4[t][ci<Cinp][co] = ci < Cin ? w[t][ci][co] : 0
__global__ void pad_cin_kernel(const float* w, float* w4, int taps, int Cin, int Cinp, int Cout)
{
    const long long total = (long long)taps * Cinp * Cout;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int co = (int)(i % Cout);
        const int ci = (int)((i / Cout) % Cinp);
        const int t = (int)(i / ((long long)Cout * Cinp));
        w4[i] = ci < Cin ? w[((long long)t * Cin + ci) * Cout + co] : 0.f;
    }
}
void launch_pad_cin(const float* w, float* w4, int taps, int Cin, int Cinp, int Cout, hipStream_t s)
{
    hipLaunchKernelGGL(pad_cin_kernel, dim3(cap_blocks((long long)taps * Cinp * Cout, 256)), dim3(256), 0, s, w, w4, taps, Cin, Cinp, Cout);
}
// wp[(py*S+px)][(t*2+v)][ci][co] = w[py+S*t][px+S*v][co][ci]   (K = 2S)
__global__ void tconv_phase_pack_kernel(const float* w, float* wp, int K, int S, int C)
{
    const long long total = (long long)S * S * 4 * C * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int co = (int)(i % C);
        const int ci = (int)((i / C) % C);
        const int tv = (int)((i / ((long long)C * C)) % 4);
        const int ph = (int)(i / ((long long)C * C * 4));
        const int py = ph / S, px = ph % S, t = tv / 2, v = tv % 2;
        const int ky = py + S * t, kx = px + S * v;
        wp[i] = w[(((long long)ky * K + kx) * C + co) * C + ci];
    }
}
void launch_tconv_phase_pack(const float* w, float* wp, int K, int S, int C, hipStream_t s)
{
    hipLaunchKernelGGL(tconv_phase_pack_kernel, dim3(cap_blocks((long long)S * S * 4 * C * C, 256)), dim3(256), 0, s, w, wp, K, S, C);
}

__global__ void dropout_mask_kernel(float* mask, long long n, float keep, unsigned long long seed, unsigned int stream)
{
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        mask[i] = philox_uniform((unsigned long long)i, seed, stream) < keep ? 1.f : 0.f;
}
void launch_dropout_mask(float* mask, long long n, float keep_prob, unsigned long long seed, unsigned int stream_id, hipStream_t s)
{
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(cap_blocks(n, 256)), dim3(256), 0, s, mask, n, keep_prob, seed, stream_id);
}

// Box-Muller normal; truncated: redraw beyond 2 sigma (tf.truncated_normal_initializer)
__global__ void init_normal_kernel(float* w, long long n, float stddev, int truncated, unsigned long long seed, unsigned int stream)
{
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float z = 0.f;
        for (int attempt = 0; attempt < 16; ++attempt) {
            const float u1 = philox_uniform((unsigned long long)i * 32 + 2 * attempt, seed, stream);
            const float u2 = philox_uniform((unsigned long long)i * 32 + 2 * attempt + 1, seed, stream);
            z = sqrtf(-2.f * logf(fmaxf(u1, 1e-12f))) * cosf(6.28318530718f * u2);
            if (!truncated || fabsf(z) <= 2.f) break;
        }
        w[i] = z * stddev;
    }
}
void launch_init_normal(float* w, long long n, float stddev, int truncated, unsigned long long seed, unsigned int stream_id, hipStream_t s)
{
    hipLaunchKernelGGL(init_normal_kernel, dim3(cap_blocks(n, 256)), dim3(256), 0, s, w, n, stddev, truncated, seed, stream_id);
}

// ---- GPU-side augmentation of a uint8 batch: per-image crop window / canvas placement, horizontal flip and
// brightness, the three geometric + photometric augmentations of data_generator/batch_generator.py:293-379 that do
// not resample.  out[n, y, x] = in[n, y + oy[n], flip ? (Wo-1-x) + ox[n] : x + ox[n]] (outside the source: image 0, label void).
// OpenCV's 8-bit RGB <-> HSV (H in [0,180)) in its own arithmetic (imgproc color_hsv: RGB2HSV_b integer path with 12-bit reciprocal
// tables, HSV2RGB_b float32 path), as restated in fcn8s_tensorflow_amd/cv2_compat.py.  The float steps use the *_rn intrinsics so that
// the compiler cannot contract a multiply and a subtract into one FMA (OpenCV's scalar code rounds after each operation).
static __device__ __forceinline__ void cv_rgb2hsv_u8(int r, int g, int b, int& h, int& s, int& v)
{
    v = max(max(r, g), b);
    const int vmin = min(min(r, g), b), diff = v - vmin;
    const int sdiv = v ? (int)rint((double)(255 << 12) / (double)v) : 0;
    const int hdiv = diff ? (int)rint((double)(180 << 12) / (6.0 * (double)diff)) : 0;
    s = (diff * sdiv + (1 << 11)) >> 12;
    int hh = v == r ? (g - b) : (v == g ? (b - r + 2 * diff) : (r - g + 4 * diff));
    hh = (hh * hdiv + (1 << 11)) >> 12;
    h = hh < 0 ? hh + 180 : hh;
}
static __device__ __forceinline__ void cv_hsv2rgb_u8(int H, int S, int V, int& r, int& g, int& b)
{
    const float s = __fmul_rn((float)S, 1.f / 255.f), v = __fmul_rn((float)V, 1.f / 255.f);
    float fb, fg, fr;
    if (s == 0.f) fb = fg = fr = v;
    else {
        float h = __fmul_rn((float)H, 6.f / 180.f);
        if (h >= 6.f) h = __fsub_rn(h, 6.f);
        int sector = (int)floorf(h);
        h = __fsub_rn(h, (float)sector);
        if ((unsigned)sector >= 6u) { sector = 0; h = 0.f; }
        const float t0 = v, t1 = __fmul_rn(v, __fsub_rn(1.f, s)), t2 = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(s, h))),
                    t3 = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(s, __fsub_rn(1.f, h))));
        switch (sector) {                      // sector_data: tab index of (b, g, r)
            case 0:  fb = t1; fg = t3; fr = t0; break;
            case 1:  fb = t1; fg = t0; fr = t2; break;
            case 2:  fb = t3; fg = t0; fr = t1; break;
            case 3:  fb = t0; fg = t2; fr = t1; break;
            case 4:  fb = t0; fg = t1; fr = t3; break;
            default: fb = t2; fg = t1; fr = t0; break;
        }
    }
    auto sat = [](float x) { const int q = (int)rintf(__fmul_rn(x, 255.f)); return q < 0 ? 0 : (q > 255 ? 255 : q); };
    r = sat(fr); g = sat(fg); b = sat(fb);
}

// crop / canvas placement, horizontal flip and brightness of data_generator/batch_generator.py:268-341, :469-486 on a uint8 batch.
// params: int[4] per image = {y offset, x offset, flip, brightness on/off}; vlut: [N][256] new V of every old V (the host evaluates the
// reference's float64 `V * random_br`, saturation and uint8 truncation once per image); brightness = RGB -> HSV, V = vlut[V], HSV -> RGB.
__global__ void augment_u8_kernel(const unsigned char* img, const unsigned char* lab, unsigned char* oimg, unsigned char* olab,
                                  const int* params, const unsigned char* vlut, int N, int H, int W, int Ho, int Wo, int void_id)
{
    const long long total = (long long)N * Ho * Wo;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wo); const long long r = i / Wo;
        const int y = (int)(r % Ho), n = (int)(r / Ho);
        const int oy = params[4 * n], ox = params[4 * n + 1], flip = params[4 * n + 2], bright = params[4 * n + 3];
        const int sy = y + oy, sx = (flip ? Wo - 1 - x : x) + ox;
        const bool in = (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W;
        const long long src = ((long long)n * H + sy) * W + sx;
        int pr = 0, pg = 0, pb = 0;
        if (in) { pr = img[src * 3]; pg = img[src * 3 + 1]; pb = img[src * 3 + 2]; }
        if (bright && vlut) {              // (the reference brightens before it flips and after it crops: canvas pixels are black and stay black)
            int h, s_, v;
            cv_rgb2hsv_u8(pr, pg, pb, h, s_, v);
            cv_hsv2rgb_u8(h, s_, vlut[n * 256 + v], pr, pg, pb);
        }
        oimg[i * 3] = (unsigned char)pr; oimg[i * 3 + 1] = (unsigned char)pg; oimg[i * 3 + 2] = (unsigned char)pb;
        if (lab) olab[i] = in ? lab[src] : (unsigned char)void_id;
    }
}
void launch_augment_u8(const unsigned char* img, const unsigned char* lab, unsigned char* oimg, unsigned char* olab, const int* params,
                       const unsigned char* vlut, int N, int H, int W, int Ho, int Wo, int void_id, hipStream_t s)
{
    hipLaunchKernelGGL(augment_u8_kernel, dim3(cap_blocks((long long)N * Ho * Wo, 256)), dim3(256), 0, s, img, lab, oimg, olab, params, vlut, N, H, W, Ho, Wo, void_id);
}


// ---- GPU-side resampling augmentations of a uint8 batch: resize, random scale, translate of
// data_generator/batch_generator.py:328-384 in one kernel.  Per image n: the source [H,W] is (virtually) resized to [rh,rw] -- images
// as cv2.resize(INTER_LINEAR) does for 8-bit data, labels as cv2.resize(INTER_NEAREST) does (both restated from OpenCV's resize.cpp in
// fcn8s_tensorflow_amd/cv2_compat.py, which this kernel matches bit for bit) -- and placed with its top-left corner at (oy,ox) of the
// [Ho,Wo] output (negative = crop); pixels not covered get 0 / void_id.
//   resize to (h',w')        : rh = Ho = h', rw = Wo = w', offset 0
//   scale by f <= 1 / f > 1  : rh = int(H f), rw = int(W f), offset = +/- |int((H - rh) / 2)| ...
//   translate by (dx,dy)     : rh = H, rw = W (exact copy), offset = (dy,dx)
// The arithmetic of both interpolations: cv_resize.h.
__global__ __launch_bounds__(256) void resample_u8_kernel(const unsigned char* __restrict__ img, const unsigned char* __restrict__ lab,
                                                          unsigned char* __restrict__ oimg, unsigned char* __restrict__ olab,
                                                          const int* __restrict__ params, int N, int H, int W, int Ho, int Wo, int void_id)
{
    const long long total = (long long)N * Ho * Wo;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wo); const long long r = i / Wo;
        const int y = (int)(r % Ho), n = (int)(r / Ho);
        const int rh = params[4 * n], rw = params[4 * n + 1], oy = params[4 * n + 2], ox = params[4 * n + 3];
        const int ry = y - oy, rx = x - ox;
        if ((unsigned)ry >= (unsigned)rh || (unsigned)rx >= (unsigned)rw) {
            if (oimg) { oimg[i * 3] = 0; oimg[i * 3 + 1] = 0; oimg[i * 3 + 2] = 0; }
            if (olab) olab[i] = (unsigned char)void_id;
            continue;
        }
        if (olab) olab[i] = lab[((long long)n * H + cv_nearest_index(ry, H, rh)) * W + cv_nearest_index(rx, W, rw)];
        if (!oimg) continue;
        int rgb[3];
        cv_resize_linear_px(img + (long long)n * H * W * 3, H, W, rh, rw, ry, rx, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) oimg[i * 3 + c] = (unsigned char)rgb[c];
    }
}
void launch_resample_u8(const unsigned char* img, const unsigned char* lab, unsigned char* oimg, unsigned char* olab, const int* params,
                        int N, int H, int W, int Ho, int Wo, int void_id, hipStream_t s)
{
    hipLaunchKernelGGL(resample_u8_kernel, dim3(cap_blocks((long long)N * Ho * Wo, 256)), dim3(256), 0, s, img, lab, oimg, olab, params,
                       N, H, W, Ho, Wo, void_id);
}


// ---- strided fingerprint of a float buffer (frozen-parameter guard): wrapping sum of the bit patterns of every 509th element ----
// (every 61st touched a different 128-byte line per sample -- 280 MB for the 134 M parameters, 57 us of a 2 ms batch-1 inference; 264 k samples
//  still see any optimizer step or whole-tensor copy, which is what the guard is for)
__global__ __launch_bounds__(256) void fingerprint_kernel(const unsigned* __restrict__ x, long long n, unsigned long long* out)
{
    unsigned long long acc = 0;
    for (long long i = (blockIdx.x * (long long)blockDim.x + threadIdx.x) * 509; i < n; i += (long long)gridDim.x * blockDim.x * 509)
        acc += (unsigned long long)x[i] * (unsigned long long)((i & 1023) + 1);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}
void launch_fingerprint(const float* x, long long n, unsigned long long* out, hipStream_t s)
{
    hipMemsetAsync(out, 0, sizeof(unsigned long long), s);
    hipLaunchKernelGGL(fingerprint_kernel, dim3(256), dim3(256), 0, s, (const unsigned*)x, n, out);
}

}  // namespace fcn8s
