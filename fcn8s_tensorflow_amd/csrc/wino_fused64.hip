// conv1_2's forward in one kernel: the 64 position GEMMs of F(6x6,3x3), 64 -> 64 channels, with the output transform, bias, ReLU and the
// 2x2/2 max-pool behind them.  M [64][T][64] -- 3.86 GB at 16 x 1024x512, written by the GEMM only for the output transform to read it back --
// never exists.  Measured first as tools/labs/fused64_lab.hip (profiles/r04_fused64_lab.txt).
//
// One block of 512 lanes owns ALL 64 positions of 16 consecutive tiles.  Wave w multiplies the eight positions of patch row w:
// 8 positions x 4 column blocks of v_mfma_f32_16x16x4_f32 accumulators, 128 registers per lane.  Operands go from global memory / L2 straight
// into the MFMA: V with one 16-byte load per lane and granule (a granule = one position x 16 input channels), the filter bank from the second,
// MFMA-ordered copy wino_filter_kernel writes for this layer, [pos][kc][nb][lane][s] = U[pos][16 kc + 4 (lane / 16) + s][16 nb + lane % 16].
// The accumulators then go through LDS in two passes of 32 channels to an epilogue in which a lane is one (tile, channel): the fma chains of
// wino_output_kernel<6, .., POOL> in their order (q = A^T M column by column, bias + sum, ReLU, first-maximum argmax byte, byte 4 when the
// maximum is not > 0, the rule for partial edge tiles), so the only arithmetic difference from the two-kernel route is the GEMM's summation order
// (k ascending in steps of one here; the LDS-DMA GEMM's own order there).
// A tile's arithmetic depends on its own V rows alone: which block holds it, and with which neighbours, changes nothing -- an image's result does
// not depend on its batch.
#include "fcn8s_internal.h"

namespace fcn8s {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// A^T of F(6,3) on the points 0, 1, -1, 2, -2, 1/2, -1/2, inf: WinoMat<6, 3>::at of winograd.hip, value for value (the two epilogues must
// multiply by the same constants in the same order)
static __device__ __forceinline__ float at63(int i, int j)
{
    constexpr float m[6][8] = {{1, 1, 1, 1, 1, 1, 1, 0}, {0, 1, -1, 2, -2, 1.f / 2, -1.f / 2, 0}, {0, 1, 1, 4, 4, 1.f / 4, 1.f / 4, 0},
                               {0, 1, -1, 8, -8, 1.f / 8, -1.f / 8, 0}, {0, 1, 1, 16, 16, 1.f / 16, 1.f / 16, 0}, {0, 1, -1, 32, -32, 1.f / 32, -1.f / 32, 1}};
    return m[i][j];
}

constexpr int kF64Tiles = 16;            // tiles per block (the 16 rows of the MFMA)
constexpr int kF64Lt = 33;               // LDS row: 32 channels + 1 pad
constexpr int kF64Dist = 2;              // prefetch distance in granules (lab: 1.52 ms at 2, 1.56 / 1.57 / 1.62 at 1 / 3 / 4)
constexpr size_t kF64LdsBytes = (size_t)64 * kF64Tiles * kF64Lt * sizeof(float);      // 132 KB: one block per CU

// v [64][T][64] slabs `slab` floats apart, up: the MFMA-ordered bank, bias [64]; pool [N, H/2, W/2, 64], pidx (may be null) one byte per pooled element
template <bool NT>
__global__ __launch_bounds__(512, 1) void wino_gemm_out64_kernel(const float* __restrict__ v, const float* __restrict__ up, const float* __restrict__ bias,
                                                                 float* __restrict__ pool, unsigned char* __restrict__ pidx,
                                                                 int N, int H, int W, long long T, long long slab)
{
    extern __shared__ float lds[];
    constexpr int D = kF64Dist, LT = kF64Lt;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long t0 = (long long)blockIdx.x * kF64Tiles;
    const int ti = lane & 15, q = lane >> 4;
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // the last block may own fewer than 16 tiles: its spare rows read tile T - 1 again and are never stored
    const long long trow = t0 + ti < T ? t0 + ti : T - 1;
    const float* vbase = v + (long long)(8 * wave) * slab + trow * 64 + q * 4;
    const float* ubase = up + (long long)(8 * wave) * 4096 + lane * 4;
    // granule g = (position 8 wave + g / 4, channel chunk g % 4): one 16-byte A load and four 16-byte B loads per lane, 16 MFMAs.  Loads return in
    // issue order, so the HBM-latency A loads and the L2-latency B loads share one prefetch distance.
    f32x4 ra[D + 1], rb[D + 1][4];
    auto issue = [&](int g) {
        const int npi = g >> 2, nkc = g & 3, sl = g % (D + 1);
        ra[sl] = *reinterpret_cast<const f32x4*>(vbase + npi * slab + nkc * 16);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) rb[sl][nb] = *reinterpret_cast<const f32x4*>(ubase + ((npi * 4 + nkc) * 4 + nb) * 256);
    };
#pragma unroll
    for (int g = 0; g < D; ++g) issue(g);
#pragma unroll
    for (int g = 0; g < 32; ++g) {
        if (g + D < 32) issue(g + D);
        __builtin_amdgcn_sched_barrier(0);            // (without the barriers the compiler sinks the loads next to their use: every distance compiles to the same code, 2.05 instead of 1.52 ms)
        const int pi = g >> 2, sl = g % (D + 1);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[pi][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[sl][s], rb[sl][nb][s], acc[pi][nb], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    // acc[pi][nb][r] = M[position 8 wave + pi][tile 4 q + r][channel 16 nb + ti]
    // epilogue lane = (tile tl, channel 32 half + c)
    const int tl = tid >> 5, c = tid & 31;
    const int th = (H + 5) / 6, tw = (W + 5) / 6, Hp = H / 2, Wp = W / 2;
    const long long t = t0 + tl;
    const bool ok = t < T;
    const long long tc = ok ? t : T - 1;
    const int n = (int)(tc / ((long long)th * tw)), rem = (int)(tc - (long long)n * th * tw), ty = rem / tw, tx = rem - ty * tw;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half) __syncthreads();                    // every lane has read the first half back
#pragma unroll
        for (int pi = 0; pi < 8; ++pi)
#pragma unroll
            for (int nb2 = 0; nb2 < 2; ++nb2)
#pragma unroll
                for (int r = 0; r < 4; ++r) lds[((8 * wave + pi) * kF64Tiles + 4 * q + r) * LT + 16 * nb2 + ti] = acc[pi][2 * half + nb2][r];
        __syncthreads();
        const int ch = 32 * half + c;
        const float* mp = lds + tl * LT + c;
        float qv[6][8];                               // q = A^T M, column by column
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            float col[8];
#pragma unroll
            for (int a = 0; a < 8; ++a) col[a] = mp[(a * 8 + b) * kF64Tiles * LT];
#pragma unroll
            for (int o = 0; o < 6; ++o) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) if (at63(o, k) != 0.f) s = fmaf(at63(o, k), col[k], s);
                qv[o][b] = s;
            }
        }
        const float bv = bias[ch];
        float pmax[3][3]; unsigned char parg[3][3];
#pragma unroll
        for (int oy = 0; oy < 6; ++oy)
#pragma unroll
            for (int ox = 0; ox < 6; ++ox) {
                float y = bv;
#pragma unroll
                for (int k = 0; k < 8; ++k) if (at63(ox, k) != 0.f) y = fmaf(at63(ox, k), qv[oy][k], y);
                const int py = oy / 2, px = ox / 2;
                const bool inside = 6 * ty + oy < H && 6 * tx + ox < W;              // false only in partial edge tiles
                if (!inside) { if ((oy & 1) == 0 && (ox & 1) == 0) { pmax[py][px] = y; parg[py][px] = 0; } continue; }
                y = fmaxf(y, 0.f);
                if ((oy & 1) == 0 && (ox & 1) == 0) { pmax[py][px] = y; parg[py][px] = 0; }
                else if (y > pmax[py][px]) { pmax[py][px] = y; parg[py][px] = (unsigned char)((oy & 1) * 2 + (ox & 1)); }
            }
        if (ok) {
#pragma unroll
            for (int py = 0; py < 3; ++py)
#pragma unroll
                for (int px = 0; px < 3; ++px)
                    if (3 * ty + py < Hp && 3 * tx + px < Wp) {                      // H, W even: a window is inside or outside as a whole
                        const long long po = (((long long)n * Hp + 3 * ty + py) * Wp + 3 * tx + px) * 64 + ch;
                        if constexpr (NT) __builtin_nontemporal_store(pmax[py][px], pool + po); else pool[po] = pmax[py][px];
                        if (pidx) pidx[po] = pmax[py][px] > 0.f ? parg[py][px] : (unsigned char)4;
                    }
        }
    }
}

size_t wino_gemm_out64_bank_floats() { return (size_t)64 * 64 * 64; }

// false: not launched (the caller runs the position GEMM and the output transform)
// nt: -1 = the size rule below picks the non-temporal instantiation; 0 / 1 = the caller does (the op-level entry points, for their small shapes)
bool launch_wino_gemm_out64(const float* v, const float* up, const float* bias, float* pool, unsigned char* pidx, int N, int H, int W, hipStream_t s, int nt)
{
    if (!v || !up || !bias || !pool || N <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2) return false;
    const long long T = (long long)N * ((H + 5) / 6) * ((W + 5) / 6);
    const long long blocks = (T + kF64Tiles - 1) / kF64Tiles;
    if (blocks > 0x7fffffffLL) return false;
    const bool big = nt >= 0 ? nt != 0 : (double)N * H * W * 64 >= 64e6;          // launch_wino_output's rule: bytes of the pool this launch writes
    const hipError_t e = hipFuncSetAttribute(big ? reinterpret_cast<const void*>(&wino_gemm_out64_kernel<true>) : reinterpret_cast<const void*>(&wino_gemm_out64_kernel<false>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kF64LdsBytes);
    if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "wino_gemm_out64: %zu bytes of LDS refused (%s)", kF64LdsBytes, hipGetErrorString(e)); return false; }
    g_last_kernel = "wino_gemm_out64_kernel";
    if (big) hipLaunchKernelGGL(wino_gemm_out64_kernel<true>, dim3((unsigned)blocks), dim3(512), kF64LdsBytes, s, v, up, bias, pool, pidx, N, H, W, T, wino_slab(T, 64));
    else     hipLaunchKernelGGL(wino_gemm_out64_kernel<false>, dim3((unsigned)blocks), dim3(512), kF64LdsBytes, s, v, up, bias, pool, pidx, N, H, W, T, wino_slab(T, 64));
    return true;
}

}  // namespace fcn8s
