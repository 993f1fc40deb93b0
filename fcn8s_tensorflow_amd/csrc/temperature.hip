// Temperature scaling of a softmax (fcn8s_op_temperature_nll, fcn8s_op_temperature_apply; the definition is in fcn8s_hip.h):
//   temperature_nll_kernel    one pass over the N * P pixels that evaluates the NLL of the calibrated distribution for K candidate beta = 1 / T
//                             at once: the 4 C bytes of a row and the label byte are read once, the C logarithms are taken once, and every
//                             candidate costs C x (multiply, v_exp_f32, add) plus one logf.  Integer tables: any order of pixels gives the same bits.
//   temperature_apply_kernel  q = the calibrated distribution (in place or not) and / or its entropy h(q).
//
// Loads (both kernels): the scheme of reliability.hip, restated here rather than shared through a header so that reliability.hip and its object
// stay byte for byte what they were.  A block of 256 threads takes a tile of 256 consecutive pixels per trip; the tile's 256 C floats come in with
// lane-contiguous loads (16 bytes per lane when the pointers are 16-byte aligned and C % 4 == 0, else 4 bytes), land in an LDS image [256][S]
// and are read back one row per thread.  S = C if C / 4 is odd, else C + 4, on the 16-byte path (ds_read_b128 without conflicts; S = 20 for C = 20);
// S = C if C is odd, else C + 1, on the generic path (ds_read_b32 at an odd stride).  With C == 20 on the 16-byte path the next tile's loads are
// issued into registers before the current tile is worked on.  S > 64 does not fit the image: such rows are read from global memory, a thread
// per row (correct, not fast; the logarithms are then taken again in the second sweep).
//
// A thread owns its row of the image: it overwrites p_c by l_c = logf(max(p_c, FLT_MIN)) in the first sweep (which also finds m and any
// non-finite p_c), and the second sweep reads d_c = l_c - m once per class for all candidates.  temperature_apply writes e_c, then q_c, into the
// same row, and the block stores the image with the lane-contiguous pattern it was loaded with.
//
// The exponential.  e_c = expf(beta * d_c) is evaluated as v_exp_f32(beta2 * d_c) with beta2 = fl(beta * log2(e)) formed on the host: the inner
// loop is then exactly multiply + v_exp_f32 + add.  Against expf the argument carries a relative error of 2^-23 (beta2's rounding and the
// product's), which moves e_c by at most |x| e^x 2^-23 <= 0.37 * 2^-23 absolute (x = beta d_c <= 0) -- below half an ulp of s >= 1 per class -- and
// v_exp_f32 itself is good to 1 ulp.  In units of 2^-16 of the NLL that is < 0.01 per pixel, against a float32-to-float64 distance of 0.1 .. 0.5.
// d of the argmax is exactly 0 and v_exp_f32(0) is exactly 1, so s >= 1 and nll >= 0 hold.  Both kernels use the same function (ts_exp), so
// reliability_pair on temperature_apply's output sees the distribution whose NLL temperature_nll summed.
//
// Counting (temperature_nll).  K is rounded up to KB in {1, 2, 4, 8, 16, 32}, a template parameter: the candidate loop is unrolled, the running
// sums s[KB] and the 64-bit accumulators acc[KB] are registers, beta and beta2 are kernel arguments (scalar registers); the padding candidates
// repeat the last beta and are not flushed.  Per-thread 64-bit sums over the block's trips, one wave reduction and one LDS atomic per candidate at
// block end, then one global 64-bit atomic per non-zero entry.
#include "fcn8s_internal.h"
#include "entropy_term.h"
#include <cfloat>
#include <cmath>

namespace fcn8s {

#define TS_THREADS FCN8S_TS_TILE_PIXELS
#define TS_KMAX FCN8S_TS_MAX_CANDIDATES
#define TS_MAX_STRIDE 64                             // floats per row of the LDS image: 64 KB for the tile

// row stride of the LDS image on the 16-byte path (the header comment has the rule)
__host__ __device__ constexpr int ts_vec_stride(int C) { return (C / 4) & 1 ? C : C + 4; }

static __device__ __forceinline__ float ts_exp(float beta2, float d)
{
#pragma clang fp contract(off)
    const float x = beta2 * d;
    return __builtin_amdgcn_exp2f(x);
}

// what a thread holds of a tile before it is worked on: (NV > 0) its NV 16-byte pieces of the tile's rows, and its label byte
template <int NV>
struct TsIn {
    float4 pv[NV > 0 ? NV : 1];
    unsigned int g;
};

// T: pixels in all; gt may be null (temperature_apply)
template <int NV>
__device__ __forceinline__ void ts_load(const float* prob, const uint8_t* gt, long long T, long long tile, int t, TsIn<NV>& in)
{
    const long long g0 = tile * TS_THREADS;
    const long long left = T - g0;
    const int npx = left < TS_THREADS ? (int)left : TS_THREADS;
    if (NV > 0) {
        const float4* src = reinterpret_cast<const float4*>(prob + g0 * (NV * 4));
        const int nvec = npx * NV;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = t + k * TS_THREADS;
            in.pv[k] = i < nvec ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    in.g = 255u;
    if (gt && t < npx) in.g = gt[g0 + t];
}

// the tile's npx rows of C floats at src into the image [TS_THREADS][S] (S > 0)
template <bool VEC, int NV>
__device__ __forceinline__ void ts_fill(float* stage, const TsIn<NV>& in, const float* src, int npx, int C, int S, int t)
{
    if (NV > 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int f = (t + k * TS_THREADS) * 4, px = f / C, c = f - px * C;                 // px < 256 for every k < NV
            *reinterpret_cast<float4*>(stage + px * S + c) = in.pv[k];
        }
    } else if (VEC) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const int nvec = npx * (C / 4);
        for (int i = t; i < nvec; i += TS_THREADS) {
            const int f = i * 4, px = f / C, c = f - px * C;
            *reinterpret_cast<float4*>(stage + px * S + c) = s4[i];
        }
    } else {
        const int nfl = npx * C, dq = TS_THREADS / C, dr = TS_THREADS % C;
        int px = t / C, c = t - px * C;
        for (int i = t; i < nfl; i += TS_THREADS) {
            stage[px * S + c] = src[i];
            px += dq; c += dr;
            if (c >= C) { c -= C; ++px; }
        }
    }
}

// the inverse of ts_fill: the image's first npx rows to dst, lane-contiguous
template <bool VEC>
__device__ __forceinline__ void ts_drain(const float* stage, float* dst, int npx, int C, int S, int t)
{
    if (VEC) {
        float4* d4 = reinterpret_cast<float4*>(dst);
        const int nvec = npx * (C / 4);
        for (int i = t; i < nvec; i += TS_THREADS) {
            const int f = i * 4, px = f / C, c = f - px * C;
            d4[i] = *reinterpret_cast<const float4*>(stage + px * S + c);
        }
    } else {
        const int nfl = npx * C, dq = TS_THREADS / C, dr = TS_THREADS % C;
        int px = t / C, c = t - px * C;
        for (int i = t; i < nfl; i += TS_THREADS) {
            dst[i] = stage[px * S + c];
            px += dq; c += dr;
            if (c >= C) { c -= C; ++px; }
        }
    }
}

// First sweep over a row: l_c = logf(max(p_c, FLT_MIN)), m = max_c l_c; false if a p_c is NaN or +-inf (tested on p_c: fmaxf hides a NaN).
// WRITE: the row is the thread's own row of the image and p_c is overwritten by l_c; otherwise (a row in global memory) nothing is written.
template <bool VEC, bool WRITE>
__device__ __forceinline__ bool ts_logs(float* row, const float* grow, int C, float& m)
{
    bool fin = true; float mx = -INFINITY;
    if (VEC) {
        float4* r4 = reinterpret_cast<float4*>(__builtin_assume_aligned(row, 16));
        const int n4 = C / 4;
        for (int i = 0; i < n4; ++i) {
            const float4 q = r4[i];
            float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                fin = fin && isfinite(v[j]);
                v[j] = logf(fmaxf(v[j], FLT_MIN));
                mx = fmaxf(mx, v[j]);
            }
            r4[i] = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const float p = WRITE ? row[c] : grow[c];
            fin = fin && isfinite(p);
            const float l = logf(fmaxf(p, FLT_MIN));
            mx = fmaxf(mx, l);
            if (WRITE) row[c] = l;
        }
    }
    m = mx;
    return fin;
}

__device__ __forceinline__ unsigned long long ts_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned long long)__shfl_down((long long)v, d, 64);
    return v;
}

struct TsNllArgs {
    const float* prob; const uint8_t* gt; const uint8_t* lut;
    long long T;                                     // N * P
    int C, S, K;                                     // S: row stride of the LDS image in floats, 0 = rows are read from global memory
    float beta[TS_KMAX], beta2[TS_KMAX];             // beta2 = fl(beta * log2(e)); entries K .. KB - 1 repeat entry K - 1
    unsigned long long *nll, *count, *bad;
};

// grid: blocks (<= tiles), block: TS_THREADS.  VEC: the 16-byte path; CT: C as a compile-time constant (next-tile loads in registers), 0 = a.C;
// KB: candidates evaluated (K rounded up)
template <bool VEC, int CT, int KB>
__global__ __launch_bounds__(TS_THREADS) void temperature_nll_kernel(const TsNllArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long ts_lds[];
    constexpr int NV = CT / 4;
    const int t = threadIdx.x, lane = t & 63;
    const int C = CT > 0 ? CT : a.C, S = CT > 0 ? ts_vec_stride(CT) : a.S;
    unsigned long long* red = ts_lds;                                                           // [TS_KMAX + 3] (+ 5 of padding)
    uint8_t* lut = reinterpret_cast<uint8_t*>(red + TS_KMAX + 8);                               // [256]
    float* stage = reinterpret_cast<float*>(lut + 256);                                         // [TS_THREADS][S]: every offset a multiple of 16 bytes
    if (t < TS_KMAX + 8) red[t] = 0ull;
    lut[t] = a.lut[t];                                                                          // TS_THREADS == 256 entries
    __syncthreads();

    const long long tiles = (a.T + TS_THREADS - 1) / TS_THREADS;
    unsigned long long acc[KB], n_all = 0, bad0 = 0, bad1 = 0;
#pragma unroll
    for (int k = 0; k < KB; ++k) acc[k] = 0ull;
    TsIn<NV> in;
    if ((long long)blockIdx.x < tiles) ts_load<NV>(a.prob, a.gt, a.T, blockIdx.x, t, in);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long g0 = tile * TS_THREADS;
        const long long left = a.T - g0;
        const int npx = left < TS_THREADS ? (int)left : TS_THREADS;
        if (S > 0) {
            ts_fill<VEC, NV>(stage, in, a.prob + g0 * C, npx, C, S, t);
            __syncthreads();
        }
        const unsigned int gtv = in.g;
        const long long next = tile + gridDim.x;
        if (next < tiles) ts_load<NV>(a.prob, a.gt, a.T, next, t, in);                          // in flight while this tile is worked on

        const unsigned int tc = t < npx ? lut[gtv & 0xFFu] : 255u;
        if (tc != 255u) {
            if (tc >= (unsigned int)C) {
                ++bad0;
            } else {
#pragma clang fp contract(off)
                float* row = stage + t * S;                                                     // used only when S > 0
                const float* grow = a.prob + (g0 + t) * C;                                      // used only when S == 0
                float m;
                const bool fin = S > 0 ? ts_logs<VEC, true>(row, grow, C, m) : ts_logs<false, false>(row, grow, C, m);
                if (!fin) {
                    ++bad1;
                } else {
                    float s[KB], dt = 0.f;
#pragma unroll
                    for (int k = 0; k < KB; ++k) s[k] = 0.f;
                    if (VEC) {
                        const float4* r4 = reinterpret_cast<const float4*>(__builtin_assume_aligned(row, 16));
                        const int n4 = C / 4;
                        for (int i = 0; i < n4; ++i) {
                            const float4 q = r4[i];
                            const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const float d = v[j] - m;
                                if (4 * i + j == (int)tc) dt = d;
#pragma unroll
                                for (int k = 0; k < KB; ++k) s[k] = s[k] + ts_exp(a.beta2[k], d);
                            }
                        }
                    } else {
                        for (int c = 0; c < C; ++c) {
                            const float l = S > 0 ? row[c] : logf(fmaxf(grow[c], FLT_MIN));
                            const float d = l - m;
                            if (c == (int)tc) dt = d;
#pragma unroll
                            for (int k = 0; k < KB; ++k) s[k] = s[k] + ts_exp(a.beta2[k], d);
                        }
                    }
                    ++n_all;
#pragma unroll
                    for (int k = 0; k < KB; ++k) {
                        const float bd = a.beta[k] * dt;
                        const float v = logf(s[k]) - bd;
                        acc[k] += (unsigned long long)(long long)rintf(v * 65536.f);
                    }
                }
            }
        }
        if (S > 0) __syncthreads();                                                            // the image is free for the next tile
    }

#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const unsigned long long r = ts_wave_sum(acc[k]);
        if (lane == 0 && r && k < a.K) atomicAdd(&red[k], r);
    }
    unsigned long long r3[3] = {n_all, bad0, bad1};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r3[i] = ts_wave_sum(r3[i]);
        if (lane == 0 && r3[i]) atomicAdd(&red[TS_KMAX + i], r3[i]);
    }
    __syncthreads();
    if (t < a.K && red[t]) atomicAdd(&a.nll[t], red[t]);
    if (t == TS_KMAX && red[t]) atomicAdd(a.count, red[t]);
    if (t > TS_KMAX && t < TS_KMAX + 3 && red[t]) atomicAdd(&a.bad[t - TS_KMAX - 1], red[t]);
}

// A thread's own row of the image, p -> l -> e -> q in place; returns h(q).  A row with a non-finite p_c becomes NaN throughout.
template <bool VEC>
__device__ __forceinline__ float ts_apply_row(float* row, int C, float beta2)
{
#pragma clang fp contract(off)
    float m, s = 0.f, h = 0.f;
    const bool fin = ts_logs<VEC, true>(row, nullptr, C, m);
    const float qnan = __builtin_nanf("");
    if (VEC) {
        float4* r4 = reinterpret_cast<float4*>(__builtin_assume_aligned(row, 16));
        const int n4 = C / 4;
        for (int i = 0; i < n4; ++i) {
            const float4 q = r4[i];
            float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] = ts_exp(beta2, v[j] - m); s = s + v[j]; }
            r4[i] = make_float4(v[0], v[1], v[2], v[3]);
        }
        for (int i = 0; i < n4; ++i) {
            const float4 q = r4[i];
            float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] = fin ? v[j] / s : qnan; h = mc_h_add(h, v[j]); }
            r4[i] = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (int c = 0; c < C; ++c) { const float e = ts_exp(beta2, row[c] - m); row[c] = e; s = s + e; }
        for (int c = 0; c < C; ++c) {
            const float q = fin ? row[c] / s : qnan;
            row[c] = q;
            h = mc_h_add(h, q);
        }
    }
    return h;
}

struct TsApplyArgs {
    const float* prob; float* out; float* ent;      // out may alias prob; out or ent may be null
    long long T;
    int C, S;
    float beta2;
};

// grid: blocks (<= tiles), block: TS_THREADS.  Template parameters as above.
template <bool VEC, int CT>
__global__ __launch_bounds__(TS_THREADS) void temperature_apply_kernel(const TsApplyArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long ts_lds[];
    constexpr int NV = CT / 4;
    const int t = threadIdx.x;
    const int C = CT > 0 ? CT : a.C, S = CT > 0 ? ts_vec_stride(CT) : a.S;
    float* stage = reinterpret_cast<float*>(ts_lds);                                            // [TS_THREADS][S]
    const float qnan = __builtin_nanf("");
    const long long tiles = (a.T + TS_THREADS - 1) / TS_THREADS;
    TsIn<NV> in;
    if ((long long)blockIdx.x < tiles) ts_load<NV>(a.prob, nullptr, a.T, blockIdx.x, t, in);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long g0 = tile * TS_THREADS;
        const long long left = a.T - g0;
        const int npx = left < TS_THREADS ? (int)left : TS_THREADS;
        if (S > 0) {
            ts_fill<VEC, NV>(stage, in, a.prob + g0 * C, npx, C, S, t);
            __syncthreads();
        }
        const long long next = tile + gridDim.x;
        if (next < tiles) ts_load<NV>(a.prob, nullptr, a.T, next, t, in);      // another tile's bytes: this block alone reads and writes its tiles

        if (t < npx) {
#pragma clang fp contract(off)
            float h = 0.f;
            if (S > 0) {
                h = ts_apply_row<VEC>(stage + t * S, C, a.beta2);
            } else {
                const float* grow = a.prob + (g0 + t) * C;
                float* orow = a.out ? a.out + (g0 + t) * C : nullptr;
                float m, unused;
                const bool fin = ts_logs<false, false>(&unused, grow, C, m);
                float s = 0.f;
                for (int c = 0; c < C; ++c) s = s + ts_exp(a.beta2, logf(fmaxf(grow[c], FLT_MIN)) - m);
                for (int c = 0; c < C; ++c) {                                                   // p_c is read before q_c takes its place
                    const float e = ts_exp(a.beta2, logf(fmaxf(grow[c], FLT_MIN)) - m);
                    const float q = fin ? e / s : qnan;
                    if (orow) orow[c] = q;
                    h = mc_h_add(h, q);
                }
            }
            if (a.ent) a.ent[g0 + t] = h;
        }
        if (S > 0) {
            __syncthreads();
            if (a.out) ts_drain<VEC>(stage, a.out + g0 * C, npx, C, S, t);
            __syncthreads();                                                                    // the image is free for the next tile
        }
    }
}

static bool ts_lds_ok(const void* fn, size_t lds, const char* what)
{
    if (lds <= 64 * 1024) return true;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "%s: %zu bytes of LDS refused (%s)", what, lds, hipGetErrorString(e)); return false; }
    return true;
}

// blocks for `tiles` tiles at `lds` bytes per block: no more than are resident at once (256 CUs, 160 KB of LDS each, at most 4 blocks per CU)
static int ts_blocks(long long tiles, size_t lds)
{
    long long blocks = tiles < FCN8S_TS_MAX_BLOCKS ? tiles : FCN8S_TS_MAX_BLOCKS;
    long long per_cu = (long long)(160 * 1024 / (lds ? lds : 1));
    per_cu = per_cu > 4 ? 4 : (per_cu < 1 ? 1 : per_cu);
    if (blocks > 256 * per_cu) blocks = 256 * per_cu;
    return (int)(blocks < 1 ? 1 : blocks);
}

// the path of a call: 16-byte loads or not, and the row stride of the LDS image (0: rows from global memory)
static void ts_path(bool aligned, int C, bool& vec, int& S)
{
    vec = aligned && C % 4 == 0;
    S = vec ? ts_vec_stride(C) : (C & 1 ? C : C + 1);
    if (S > TS_MAX_STRIDE) { S = 0; vec = false; }
}

template <bool VEC, int CT, int KB>
static void ts_nll_launch(const TsNllArgs& a, int blocks, size_t lds, hipStream_t s)
{
    if (!ts_lds_ok(reinterpret_cast<const void*>(&temperature_nll_kernel<VEC, CT, KB>), lds, "temperature_nll")) return;
    hipLaunchKernelGGL((temperature_nll_kernel<VEC, CT, KB>), dim3(blocks), dim3(TS_THREADS), lds, s, a);
}

template <int KB>
static void ts_nll_path(const TsNllArgs& a, bool vec, int blocks, size_t lds, hipStream_t s)
{
    if (vec && a.C == 20) ts_nll_launch<true, 20, KB>(a, blocks, lds, s);
    else if (vec) ts_nll_launch<true, 0, KB>(a, blocks, lds, s);
    else ts_nll_launch<false, 0, KB>(a, blocks, lds, s);
}

void launch_temperature_nll(const float* prob, const uint8_t* gt, const uint8_t* lut, int N, long long P, int C, const float* betas, int K,
                            unsigned long long* nll, unsigned long long* count, unsigned long long* bad, hipStream_t s)
{
    TsNllArgs a = {};
    a.prob = prob; a.gt = gt; a.lut = lut; a.T = (long long)N * P; a.C = C; a.K = K;
    a.nll = nll; a.count = count; a.bad = bad;
    for (int k = 0; k < TS_KMAX; ++k) {
        const float b = betas[k < K ? k : K - 1];
        a.beta[k] = b; a.beta2[k] = (float)((double)b * 1.4426950408889634);
    }
    bool vec;
    ts_path(((uintptr_t)prob & 15) == 0, C, vec, a.S);
    const size_t lds = (size_t)(TS_KMAX + 8) * 8 + 256 + (size_t)TS_THREADS * a.S * 4;
    const int blocks = ts_blocks((a.T + TS_THREADS - 1) / TS_THREADS, lds);
    if (K <= 1) ts_nll_path<1>(a, vec, blocks, lds, s);
    else if (K <= 2) ts_nll_path<2>(a, vec, blocks, lds, s);
    else if (K <= 4) ts_nll_path<4>(a, vec, blocks, lds, s);
    else if (K <= 8) ts_nll_path<8>(a, vec, blocks, lds, s);
    else if (K <= 16) ts_nll_path<16>(a, vec, blocks, lds, s);
    else ts_nll_path<32>(a, vec, blocks, lds, s);
}

template <bool VEC, int CT>
static void ts_apply_launch(const TsApplyArgs& a, int blocks, size_t lds, hipStream_t s)
{
    if (!ts_lds_ok(reinterpret_cast<const void*>(&temperature_apply_kernel<VEC, CT>), lds, "temperature_apply")) return;
    hipLaunchKernelGGL((temperature_apply_kernel<VEC, CT>), dim3(blocks), dim3(TS_THREADS), lds, s, a);
}

void launch_temperature_apply(const float* prob, int N, long long P, int C, float beta, float* out, float* entropy_out, hipStream_t s)
{
    TsApplyArgs a = {};
    a.prob = prob; a.out = out; a.ent = entropy_out; a.T = (long long)N * P; a.C = C;
    a.beta2 = (float)((double)beta * 1.4426950408889634);
    bool vec;
    ts_path((((uintptr_t)prob | (uintptr_t)out) & 15) == 0, C, vec, a.S);
    const size_t lds = (size_t)TS_THREADS * a.S * 4;
    const int blocks = ts_blocks((a.T + TS_THREADS - 1) / TS_THREADS, lds);
    if (vec && C == 20) ts_apply_launch<true, 20>(a, blocks, lds, s);
    else if (vec) ts_apply_launch<true, 0>(a, blocks, lds, s);
    else ts_apply_launch<false, 0>(a, blocks, lds, s);
}

}  // namespace fcn8s
