// fc6 (7x7 SAME, fp32 training step) through 14x14 real-DFT tiles with Gauss's three-product complex multiply.
//
// Each 14x14 input patch (origin 8t - 3, zeros outside the map) is correlated with the 7x7 filter as a circular convolution with the
// flipped filter zero-padded to 14x14; the last 8x8 of each circular output are the tile's 8x8 outputs (14 = 8 + 7 - 1), so maps tile
// at stride 8.  A 2-D real DFT of 14x14 has 196 independent real values: rfft columns v = 1..6 carry 14 complex frequencies each; columns
// 0 and 7 carry two real ones (u = 0, 7) and six complex ones (u = 1..6; u = 8..13 are their conjugates).  Per complex frequency three
// real GEMM planes (input a + b, a, b against filter c, d - c, c + d: k1, k2, k3; real = k1 - k3, imag = k1 + k2), one per real frequency:
// 96 * 3 + 4 = 292 planes, 4.56 multiplies per output and (ci, co) pair against F(4x4,4x4)'s 12.25.
//
//   forward        : Uf = filter(w), Xf = input(x), Yf[p] = Xf[p] Uf[p] (GEMM over Cin), y = output(Yf) (+ bias, ReLU, dropout)
//   data gradient  : dYf = output^T(dz), dXf[p] = dYf[p] Uf[p]^T (same bank, read transposed), dx = input^T(dXf)
//   weight gradient: dUf[p] = Xf[p]^T dYf[p] (the forward's Xf, the data gradient's dYf), dw = filter^T(dUf)
//
// The adjoint transforms are the exact transposes of the forward ones (the inverse real DFT weighs every frequency that has a conjugate
// partner twice; its transpose keeps that factor, the forward DFT of the input has none).  tools/fft_fc6_probe.py and
// tests/test_fc6_fft_host.py hold a float64 model of the same plane set.
// Plane order: complex frequency f (96) -> planes 3f, 3f + 1, 3f + 2; f = u - 1 in column 0 (u = 1..6), 6 + 14 (v - 1) + u in columns
// 1..6, 90 + u - 1 in column 7; real planes 288 + (u == 7) + 2 (v == 7).  Slabs of [P][T][C] tensors are wino_slab(T, C) apart.
// All kernels are element-wise along the channel axis (one channel per lane, coalesced 4-byte accesses); twiddles fold into immediates.
#include "fcn8s_internal.h"

namespace fcn8s {

namespace {

__device__ __forceinline__ float c14(int k)
{
    constexpr float t[14] = {1.000000000f, 0.900968868f, 0.623489802f, 0.222520934f, -0.222520934f, -0.623489802f, -0.900968868f,
                             -1.000000000f, -0.900968868f, -0.623489802f, -0.222520934f, 0.222520934f, 0.623489802f, 0.900968868f};
    return t[k % 14];
}
__device__ __forceinline__ float s14(int k)
{
    constexpr float t[14] = {0.000000000f, 0.433883739f, 0.781831482f, 0.974927912f, 0.974927912f, 0.781831482f, 0.433883739f,
                             0.000000000f, -0.433883739f, -0.781831482f, -0.974927912f, -0.974927912f, -0.781831482f, -0.433883739f};
    return t[k % 14];
}
constexpr int nu_of(int v) { return (v == 0 || v == 7) ? 8 : 14; }                                  // stored rows u of column v
constexpr bool is_real(int u, int v) { return (v == 0 || v == 7) && (u == 0 || u == 7); }
constexpr int cplx(int u, int v) { return v == 0 ? u - 1 : (v == 7 ? 90 + u - 1 : 6 + (v - 1) * 14 + u); }
constexpr int realp(int u, int v) { return 288 + (u == 7 ? 1 : 0) + (v == 7 ? 2 : 0); }

#define FFT_FENCE __builtin_amdgcn_sched_barrier(0)

inline int grid_for(long long work)
{
    const long long b = (work + 255) / 256;
    return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}

// ---- filter bank: w[7][7][Cin][Cout] -> uf[292][Cin][Cout] ------------------------------------------------------------------
template <int V>
__device__ __forceinline__ void filter_col(const float (&g)[7][7], float* __restrict__ uf, long long e, long long CC)
{
    float rr[7], ri[7];                                       // row DFT of the flipped filter wf[a][b] = g[6 - a][6 - b], column V
#pragma unroll
    for (int a = 0; a < 7; ++a) {
        float sr = 0.f, si = 0.f;
#pragma unroll
        for (int b = 0; b < 7; ++b) { sr = fmaf(g[6 - a][6 - b], c14(V * b), sr); si = fmaf(g[6 - a][6 - b], -s14(V * b), si); }
        rr[a] = sr; ri[a] = si;
    }
#pragma unroll
    for (int u = 0; u < nu_of(V); ++u) {
        float cr = 0.f, ci = 0.f;
#pragma unroll
        for (int a = 0; a < 7; ++a) {
            cr = fmaf(rr[a], c14(u * a), fmaf(ri[a], s14(u * a), cr));
            ci = fmaf(ri[a], c14(u * a), fmaf(rr[a], -s14(u * a), ci));
        }
        if (is_real(u, V)) uf[realp(u, V) * CC + e] = cr;
        else {
            const long long p = 3LL * cplx(u, V) * CC + e;
            uf[p] = cr; uf[p + CC] = ci - cr; uf[p + 2 * CC] = cr + ci;
        }
    }
}
__global__ __launch_bounds__(256) void fft_fc6_filter_kernel(const float* __restrict__ w, float* __restrict__ uf, long long CC)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < CC; e += (long long)gridDim.x * 256) {
        float g[7][7];
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int b = 0; b < 7; ++b) g[a][b] = w[(a * 7 + b) * CC + e];
        filter_col<0>(g, uf, e, CC); filter_col<1>(g, uf, e, CC); filter_col<2>(g, uf, e, CC); filter_col<3>(g, uf, e, CC);
        filter_col<4>(g, uf, e, CC); filter_col<5>(g, uf, e, CC); filter_col<6>(g, uf, e, CC); filter_col<7>(g, uf, e, CC);
    }
}

// ---- transpose of the filter transform: duf[292][Cin][Cout] -> dw[7][7][Cin][Cout] (weight gradient) ---------------------
// Gauss stage: uf = (cr, ci - cr, cr + ci) -> dcr = d0 - d1 + d2, dci = d1 + d2; real planes pass through.  The filter transform is a plain
// forward DFT (the conjugate-pair factor beta / 196 lives in the output transform, so dYf and hence dUf already carry it): no factor here.
// Column V: dr[a] = sum_u dcr cos(u a) - dci sin(u a), di[a] = sum_u dcr sin(u a) + dci cos(u a); dg[6 - a][6 - b] += dr[a] cos(V b) - di[a] sin(V b).
template <int V>
__device__ __forceinline__ void dfilter_col(const float* __restrict__ duf, float (&dg)[7][7], long long e, long long CC)
{
    constexpr int NU = nu_of(V);
    float R[NU], I[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        if (is_real(u, V)) { R[u] = duf[realp(u, V) * CC + e]; I[u] = 0.f; }
        else {
            const float* p = duf + 3LL * cplx(u, V) * CC + e;
            const float d0 = p[0], d1 = p[CC], d2 = p[2 * CC];
            R[u] = d0 - d1 + d2; I[u] = d1 + d2;
        }
    }
#pragma unroll
    for (int a = 0; a < 7; ++a) {
        float dr = 0.f, di = 0.f;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (is_real(u, V)) { dr = fmaf(R[u], c14(u * a), dr); di = fmaf(R[u], s14(u * a), di); }
            else {
                dr = fmaf(R[u], c14(u * a), fmaf(I[u], -s14(u * a), dr));
                di = fmaf(R[u], s14(u * a), fmaf(I[u], c14(u * a), di));
            }
        }
#pragma unroll
        for (int b = 0; b < 7; ++b) dg[6 - a][6 - b] = fmaf(dr, c14(V * b), fmaf(di, -s14(V * b), dg[6 - a][6 - b]));
    }
}
// one lane per (ci, co), plain stores: every element of dw has one writer
__global__ __launch_bounds__(256) void fft_fc6_dfilter_kernel(const float* __restrict__ duf, float* __restrict__ dw, long long CC)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < CC; e += (long long)gridDim.x * 256) {
        float dg[7][7];
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int b = 0; b < 7; ++b) dg[a][b] = 0.f;
        dfilter_col<0>(duf, dg, e, CC); FFT_FENCE; dfilter_col<1>(duf, dg, e, CC); FFT_FENCE; dfilter_col<2>(duf, dg, e, CC); FFT_FENCE;
        dfilter_col<3>(duf, dg, e, CC); FFT_FENCE; dfilter_col<4>(duf, dg, e, CC); FFT_FENCE; dfilter_col<5>(duf, dg, e, CC); FFT_FENCE;
        dfilter_col<6>(duf, dg, e, CC); FFT_FENCE; dfilter_col<7>(duf, dg, e, CC);
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int b = 0; b < 7; ++b) dw[(a * 7 + b) * CC + e] = dg[a][b];
    }
}

// ---- input transform: x[N][H][W][C] -> xf[292][T][C]; one lane per (tile, rfft column v, channel) ---------------------------
template <int V>
__device__ __forceinline__ void input_col(const float* __restrict__ x, float* __restrict__ xf, long long slab, long long tc, int oy, int ox,
                                          int H, int W, int C, int c, long long img)
{
    float rr[14], ri[14];
#pragma unroll
    for (int n = 0; n < 14; ++n) {
        float sr = 0.f, si = 0.f;
        const int py = oy + n;
        if (py >= 0 && py < H) {
            const float* row = x + (img + (long long)py * W) * C + c;
#pragma unroll
            for (int m = 0; m < 14; ++m) {
                const int px = ox + m;
                const float val = (px >= 0 && px < W) ? row[(long long)px * C] : 0.f;
                sr = fmaf(val, c14(V * m), sr); si = fmaf(val, -s14(V * m), si);
            }
        }
        rr[n] = sr; ri[n] = si;
    }
#pragma unroll
    for (int u = 0; u < nu_of(V); ++u) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int n = 0; n < 14; ++n) {
            a = fmaf(rr[n], c14(u * n), fmaf(ri[n], s14(u * n), a));
            b = fmaf(ri[n], c14(u * n), fmaf(rr[n], -s14(u * n), b));
        }
        if (is_real(u, V)) xf[realp(u, V) * slab + tc] = a;
        else {
            const long long p = 3LL * cplx(u, V) * slab + tc;
            xf[p] = a + b; xf[p + slab] = a; xf[p + 2 * slab] = b;
        }
    }
}
__global__ __launch_bounds__(256) void fft_fc6_input_kernel(const float* __restrict__ x, float* __restrict__ xf, int N, int H, int W, int C, long long slab)
{
    const int th = (H + 7) / 8, tw = (W + 7) / 8;
    const long long total = (long long)N * th * tw * 8 * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long r = i / C;
        const int v = (int)(r % 8);
        const long long t = r / 8;
        const int tx = (int)(t % tw), ty = (int)((t / tw) % th), n = (int)(t / ((long long)tw * th));
        const long long img = (long long)n * H * W, tc = t * C + c;
        const int oy = 8 * ty - 3, ox = 8 * tx - 3;
        switch (v) {
            case 0: input_col<0>(x, xf, slab, tc, oy, ox, H, W, C, c, img); break;
            case 1: input_col<1>(x, xf, slab, tc, oy, ox, H, W, C, c, img); break;
            case 2: input_col<2>(x, xf, slab, tc, oy, ox, H, W, C, c, img); break;
            case 3: input_col<3>(x, xf, slab, tc, oy, ox, H, W, C, c, img); break;
            case 4: input_col<4>(x, xf, slab, tc, oy, ox, H, W, C, c, img); break;
            case 5: input_col<5>(x, xf, slab, tc, oy, ox, H, W, C, c, img); break;
            case 6: input_col<6>(x, xf, slab, tc, oy, ox, H, W, C, c, img); break;
            default: input_col<7>(x, xf, slab, tc, oy, ox, H, W, C, c, img); break;
        }
    }
}

// ---- output transform: yf[292][T][C] -> y[N][H][W][C] (last 8x8 of the inverse DFT) + bias, ReLU, dropout ------------------
// y[n][m] = sum over stored (u, v) of beta / 196 (R cos th - I sin th), th = 2 pi (u n + v m) / 14, beta = 1 on the four real
// frequencies, 2 elsewhere; separably: P_v[n] = sum_u beta (R cos - I sin)(u n), Q_v[n] = sum_u beta (R sin + I cos)(u n),
// y[n][m] += P_v[n] cos(v m) - Q_v[n] sin(v m).
template <int V>
__device__ __forceinline__ void output_col(const float* __restrict__ yf, long long slab, long long tc, float (&acc)[8][8])
{
    constexpr int NU = nu_of(V);
    float R[NU], I[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        if (is_real(u, V)) { R[u] = yf[realp(u, V) * slab + tc]; I[u] = 0.f; }
        else {
            const float* p = yf + 3LL * cplx(u, V) * slab + tc;
            const float k1 = p[0], k2 = p[slab], k3 = p[2 * slab];
            R[u] = k1 - k3; I[u] = k1 + k2;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int n = 6 + j;
        float P = 0.f, Q = 0.f;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const float beta = (is_real(u, V) ? 1.f : 2.f) / 196.f;
            if (is_real(u, V)) { P = fmaf(R[u], beta * c14(u * n), P); Q = fmaf(R[u], beta * s14(u * n), Q); }
            else {
                P = fmaf(R[u], beta * c14(u * n), fmaf(I[u], -beta * s14(u * n), P));
                Q = fmaf(R[u], beta * s14(u * n), fmaf(I[u], beta * c14(u * n), Q));
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j][i] = fmaf(P, c14(V * (6 + i)), fmaf(Q, -s14(V * (6 + i)), acc[j][i]));
    }
}
__device__ __forceinline__ void output_tile(const float* __restrict__ yf, const float* __restrict__ bias, float* __restrict__ y, int H, int W, int C, long long slab,
                                            long long tc, int n, int ty, int tx, int c, int relu, int dropout, float keep, unsigned long long seed, unsigned int stream_id)
{
    float acc[8][8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
    // (a scheduling fence per column: hoisting the loads of every column costs the accumulators their registers)
    output_col<0>(yf, slab, tc, acc); FFT_FENCE; output_col<1>(yf, slab, tc, acc); FFT_FENCE; output_col<2>(yf, slab, tc, acc); FFT_FENCE;
    output_col<3>(yf, slab, tc, acc); FFT_FENCE; output_col<4>(yf, slab, tc, acc); FFT_FENCE; output_col<5>(yf, slab, tc, acc); FFT_FENCE;
    output_col<6>(yf, slab, tc, acc); FFT_FENCE; output_col<7>(yf, slab, tc, acc); FFT_FENCE;
    const float bv = bias ? bias[c] : 0.f;
    const float ik = 1.f / keep;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int py = 8 * ty + j, px = 8 * tx + k;
            if (py >= H || px >= W) continue;                 // partial edge tiles
            float v = bv + acc[j][k];
            if (relu) v = fmaxf(v, 0.f);
            const long long off = (((long long)n * H + py) * W + px) * C + c;
            if (dropout) v = philox_uniform((unsigned long long)off, seed, stream_id) < keep ? v * ik : 0.f;   // the stream of every other fc6 epilogue: element index NHWC
            y[off] = v;
        }
}
// one lane per (tile, channel)
__global__ __launch_bounds__(256) void fft_fc6_output_kernel(const float* __restrict__ yf, const float* __restrict__ bias, float* __restrict__ y,
                                                             int N, int H, int W, int C, long long slab, int relu, int dropout, float keep,
                                                             unsigned long long seed, unsigned int stream_id)
{
    const int th = (H + 7) / 8, tw = (W + 7) / 8;
    const long long total = (long long)N * th * tw * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long t = i / C;
        const int tx = (int)(t % tw), ty = (int)((t / tw) % th), n = (int)(t / ((long long)tw * th));
        output_tile(yf, bias, y, H, W, C, slab, i, n, ty, tx, c, relu, dropout, keep, seed, stream_id);
    }
}

// ---- transpose of the output transform: dz[N][H][W][C] -> dyf[292][T][C] -------------------------------------------------
// dR = beta / 196 Re G, dI = beta / 196 Im G with G[u][v] = sum over the 8x8 crop of dz e^{-i th}; dk1 = dR + dI, dk2 = dI, dk3 = -dR.
template <int V>
__device__ __forceinline__ void dout_col(const float (&d)[8][8], float* __restrict__ dyf, long long slab, long long tc)
{
    float sr[8], si[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { a = fmaf(d[j][k], c14(V * (6 + k)), a); b = fmaf(d[j][k], -s14(V * (6 + k)), b); }
        sr[j] = a; si[j] = b;
    }
#pragma unroll
    for (int u = 0; u < nu_of(V); ++u) {
        const float beta = (is_real(u, V) ? 1.f : 2.f) / 196.f;
        float gr = 0.f, gi = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = 6 + j;
            gr = fmaf(sr[j], beta * c14(u * n), fmaf(si[j], beta * s14(u * n), gr));
            gi = fmaf(si[j], beta * c14(u * n), fmaf(sr[j], -beta * s14(u * n), gi));
        }
        if (is_real(u, V)) dyf[realp(u, V) * slab + tc] = gr;
        else {
            const long long p = 3LL * cplx(u, V) * slab + tc;
            dyf[p] = gr + gi; dyf[p + slab] = gi; dyf[p + 2 * slab] = -gr;
        }
    }
}
__global__ __launch_bounds__(256) void fft_fc6_dout_kernel(const float* __restrict__ dz, float* __restrict__ dyf, int N, int H, int W, int C, long long slab)
{
    const int th = (H + 7) / 8, tw = (W + 7) / 8;
    const long long total = (long long)N * th * tw * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long t = i / C;
        const int tx = (int)(t % tw), ty = (int)((t / tw) % th), n = (int)(t / ((long long)tw * th));
        float d[8][8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int py = 8 * ty + j, px = 8 * tx + k;
                d[j][k] = (py < H && px < W) ? dz[(((long long)n * H + py) * W + px) * C + c] : 0.f;
            }
        dout_col<0>(d, dyf, slab, i); dout_col<1>(d, dyf, slab, i); dout_col<2>(d, dyf, slab, i); dout_col<3>(d, dyf, slab, i);
        dout_col<4>(d, dyf, slab, i); dout_col<5>(d, dyf, slab, i); dout_col<6>(d, dyf, slab, i); dout_col<7>(d, dyf, slab, i);
    }
}

// ---- transpose of the input transform, part 1: dxf[292][T][C] -> patch gradients pt[T][14][14][C] -----------------------
// A = d(a + b) + da, B = d(a + b) + db on complex planes, A = dr, B = 0 on real ones; patch[n][m] = sum (A cos th - B sin th) over the
// stored frequencies.  One lane per (tile, channel, half of the patch rows): 7 x 14 accumulators.
template <int V, int HALF>
__device__ __forceinline__ void din_col(const float* __restrict__ dxf, long long slab, long long tc, float (&acc)[7][14])
{
    constexpr int NU = nu_of(V);
    float A[NU], B[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        if (is_real(u, V)) { A[u] = dxf[realp(u, V) * slab + tc]; B[u] = 0.f; }
        else {
            const float* p = dxf + 3LL * cplx(u, V) * slab + tc;
            const float ds = p[0], da = p[slab], db = p[2 * slab];
            A[u] = ds + da; B[u] = ds + db;
        }
    }
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        const int n = 7 * HALF + r;
        float P = 0.f, Q = 0.f;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (is_real(u, V)) { P = fmaf(A[u], c14(u * n), P); Q = fmaf(A[u], s14(u * n), Q); }
            else {
                P = fmaf(A[u], c14(u * n), fmaf(B[u], -s14(u * n), P));
                Q = fmaf(A[u], s14(u * n), fmaf(B[u], c14(u * n), Q));
            }
        }
#pragma unroll
        for (int m = 0; m < 14; ++m) acc[r][m] = fmaf(P, c14(V * m), fmaf(Q, -s14(V * m), acc[r][m]));
    }
}
template <int HALF>
__device__ __forceinline__ void din_half(const float* __restrict__ dxf, float* __restrict__ pt, long long slab, long long t, int c, int C)
{
    float acc[7][14];
#pragma unroll
    for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int m = 0; m < 14; ++m) acc[r][m] = 0.f;
    const long long tc = t * C + c;
    din_col<0, HALF>(dxf, slab, tc, acc); FFT_FENCE; din_col<1, HALF>(dxf, slab, tc, acc); FFT_FENCE; din_col<2, HALF>(dxf, slab, tc, acc); FFT_FENCE; din_col<3, HALF>(dxf, slab, tc, acc); FFT_FENCE;
    din_col<4, HALF>(dxf, slab, tc, acc); FFT_FENCE; din_col<5, HALF>(dxf, slab, tc, acc); FFT_FENCE; din_col<6, HALF>(dxf, slab, tc, acc); FFT_FENCE; din_col<7, HALF>(dxf, slab, tc, acc);
    float* o = pt + (t * 196 + 7 * HALF * 14) * C + c;
#pragma unroll
    for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int m = 0; m < 14; ++m) o[(r * 14 + m) * C] = acc[r][m];
}
__global__ __launch_bounds__(256, 2) void fft_fc6_din_kernel(const float* __restrict__ dxf, float* __restrict__ pt, long long T, int C, long long slab)
{
    const long long total = T * 2 * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long r = i / C;
        const int half = (int)(r % 2);
        const long long t = r / 2;
        if (half == 0) din_half<0>(dxf, pt, slab, t, c, C);
        else           din_half<1>(dxf, pt, slab, t, c, C);
    }
}

// ---- part 2: overlap-add of the 14x14 patch gradients at stride 8, as a gather (one lane per pixel and channel, fixed order) -----
__global__ __launch_bounds__(256) void fft_fc6_din_gather_kernel(const float* __restrict__ pt, float* __restrict__ dx, int N, int H, int W, int C)
{
    const int th = (H + 7) / 8, tw = (W + 7) / 8;
    const long long total = (long long)N * H * W * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long p = i / C;
        const int px = (int)(p % W), py = (int)((p / W) % H), n = (int)(p / ((long long)W * H));
        // tiles covering py: ty with 0 <= py + 3 - 8 ty <= 13, i.e. ty = (py + 3) / 8 and, in its first six rows, the tile above
        const int ty1 = (py + 3) / 8, tx1 = (px + 3) / 8;
        float s = 0.f;
#pragma unroll
        for (int dy = 1; dy >= 0; --dy) {
            const int ty = ty1 - dy, ry = py + 3 - 8 * ty;
            if (ty < 0 || ty >= th || ry > 13) continue;
#pragma unroll
            for (int dxo = 1; dxo >= 0; --dxo) {
                const int tx = tx1 - dxo, rx = px + 3 - 8 * tx;
                if (tx < 0 || tx >= tw || rx > 13) continue;
                s += pt[((((long long)n * th + ty) * tw + tx) * 196 + ry * 14 + rx) * C + c];
            }
        }
        dx[i] = s;
    }
}

}  // namespace

int fft_fc6_planes() { return 292; }
long long fft_fc6_tiles(int N, int H, int W) { return (long long)N * ((H + 7) / 8) * ((W + 7) / 8); }

void launch_fft_fc6_filter(const float* w, float* uf, int Cin, int Cout, hipStream_t s)
{
    const long long CC = (long long)Cin * Cout;
    hipLaunchKernelGGL(fft_fc6_filter_kernel, dim3(grid_for(CC)), dim3(256), 0, s, w, uf, CC);
}
void launch_fft_fc6_dfilter(const float* duf, float* dw, int Cin, int Cout, hipStream_t s)
{
    const long long CC = (long long)Cin * Cout;
    hipLaunchKernelGGL(fft_fc6_dfilter_kernel, dim3(grid_for(CC)), dim3(256), 0, s, duf, dw, CC);
}
void launch_fft_fc6_input(const float* x, float* xf, int N, int H, int W, int C, hipStream_t s)
{
    const long long T = fft_fc6_tiles(N, H, W);
    hipLaunchKernelGGL(fft_fc6_input_kernel, dim3(grid_for(T * 8 * C)), dim3(256), 0, s, x, xf, N, H, W, C, wino_slab(T, C));
}
void launch_fft_fc6_output(const float* yf, const float* bias, float* y, int N, int H, int W, int C, int relu, int dropout, float keep,
                           unsigned long long seed, unsigned int stream_id, hipStream_t s)
{
    const long long T = fft_fc6_tiles(N, H, W);
    hipLaunchKernelGGL(fft_fc6_output_kernel, dim3(grid_for(T * C)), dim3(256), 0, s, yf, bias, y, N, H, W, C, wino_slab(T, C), relu, dropout, keep, seed, stream_id);
}
void launch_fft_fc6_dout(const float* dz, float* dyf, int N, int H, int W, int C, hipStream_t s)
{
    const long long T = fft_fc6_tiles(N, H, W);
    hipLaunchKernelGGL(fft_fc6_dout_kernel, dim3(grid_for(T * C)), dim3(256), 0, s, dz, dyf, N, H, W, C, wino_slab(T, C));
}
void launch_fft_fc6_din(const float* dxf, float* patches, float* dx, int N, int H, int W, int C, hipStream_t s)
{
    const long long T = fft_fc6_tiles(N, H, W);
    hipLaunchKernelGGL(fft_fc6_din_kernel, dim3(grid_for(T * 2 * C)), dim3(256), 0, s, dxf, patches, T, C, wino_slab(T, C));
    hipLaunchKernelGGL(fft_fc6_din_gather_kernel, dim3(grid_for((long long)N * H * W * C)), dim3(256), 0, s, patches, dx, N, H, W, C);
}

}  // namespace fcn8s
