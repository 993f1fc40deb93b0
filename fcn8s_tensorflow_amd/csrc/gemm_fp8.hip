// FCN8S_PREC_FP8_INFER (include/fcn8s_hip.h): the inference-only e4m3 path.  Convolutions run on the block-scaled MX MFMA
// v_mfma_scale_f32_32x32x64_f8f6f4 with OCP e4m3 operands (2x the bf16 rate per clock), plus the small kernels around them: weight
// quantization (per-column exponent + the planes the convolution reads), fp32 -> padded e4m3 copies, the byte-max pool on e4m3 copies and the
// calibration maximum.
//
// Padded e4m3 copies are 64-channel planes [C / 64][N (H + 2 pad) (W + 2 pad)][64] bytes: a 64-channel row is 64 bytes, the row of the bf16
// kernels' 32-channel planes, so the LDS-DMA staging and the XOR-swizzled 64-byte LDS rows are those of gemm_bf16.hip.
// Quantized weights are K-chunk planes [K K Cin / 64][Cout][64] (one 64-byte LDS row per output channel and K-tile).
#include "fcn8s_internal.h"

namespace fcn8s {

namespace {
typedef int fp8x32 __attribute__((ext_vector_type(8)));          // 32 e4m3 values: one lane's A or B operand of the 32x32x64 MX MFMA
typedef float accx16 __attribute__((ext_vector_type(16)));

// (base and LDS offset are wave-uniform by construction; readfirstlane tells the compiler so, which the scalar operands need)
static __device__ __forceinline__ void glds16q(const void* sbase, unsigned voff, unsigned lds_byte_off)
{
    const unsigned long long a = (unsigned long long)sbase;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const void* b = (const void*)(((unsigned long long)hi << 32) | lo);
    const unsigned o = __builtin_amdgcn_readfirstlane(lds_byte_off);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(b), "s"(o) : "memory", "m0");
}
template <int N> static __device__ __forceinline__ void wait_vmq() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// q(v) of the contract: clamp to [-448, 448] (the conversion instruction's own saturation depends on its clamp bit), then round to nearest even e4m3.
// The clamp is written with comparisons, which a NaN fails: NaN stays NaN, as in the host restatement (fminf / fmaxf would turn it into -448).
// Four values -> one dword, byte k = q(v[k]).
static __device__ __forceinline__ float clamp448(float v) { return v > 448.f ? 448.f : (v < -448.f ? -448.f : v); }
static __device__ __forceinline__ unsigned q8x4(float a, float b, float c, float d)
{
    a = clamp448(a); b = clamp448(b); c = clamp448(c); d = clamp448(d);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (unsigned)w;
}

// E(a): the smallest integer e with a <= 448 2^e; E(0) = 0 (exact in double)
static __device__ __forceinline__ int fp8_exponent(float a)
{
    if (!(a > 0.f)) return 0;
    int e = ilogb((double)a) - 8;
    while ((double)a > ldexp(448.0, e)) ++e;
    while ((double)a <= ldexp(448.0, e - 1)) --e;
    return e;
}
}

// ---- the convolution -------------------------------------------------------------------------------------------------------------------
// y[m, co] = 2^(ex + ew[co]) sum_k Xq[m, k] Wq[k, co] + bias[co] (ReLU), rows m = output pixels of [N][H][W], k = (tap, channel).  A row's K-tile
// (tap (ty, tx), 64-channel chunk c) is the 64-byte row of the padded copy at the pixel's window position moved by the tap: 256 rows x 64 bytes per
// tile, gathered by LDS-DMA with 32-bit per-lane offsets from the window of the tile's first row (64-bit scalar base, as conv_bf16_256_kernel).
// One MX MFMA per 32 x 32 tile and K-tile (K = 64 channels), scale operands 2^0: the power-of-two scales are applied in the epilogue (exact).
// A and B fragments are read with the same lane / byte assignment (lane half h: logical chunks 2h, 2h + 1 of the row), so channel k of A meets
// channel k of B whatever the instruction's internal k order is; tests/test_fp8_gpu.py checks the product with exact integer data.
// Three LDS stages, tiles issued two ahead, one barrier per K-tile.  Epilogue through LDS (row-major, 8 channels per lane): fp32 store and / or the
// consumer's padded e4m3 copy q(y 2^-yq_exp).
template <int BN>
__global__ __launch_bounds__(512, 2) void conv_fp8_kernel(const Fp8ConvArgs p)
{
    constexpr int BM = 256, ROWB = 64;
    constexpr int WCN = BN / 64, WRN = 8 / WCN, TM = BM / (32 * WRN), TN = 2;        // BN 128: 4 x 2 waves of 64 x 64; BN 64: 8 x 1 waves of 32 x 64
    constexpr int ABYTES = BM * ROWB, STAGE = ABYTES + BN * ROWB, NS = 3;
    constexpr int NAI = BM / 16 / 8, NBC = BN / 16;
    __shared__ __attribute__((aligned(16))) unsigned char smem[NS * STAGE];           // 72 / 60 KB: two blocks per CU
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WCN, wn = wave % WCN;
    const int pad = (p.K - 1) / 2, Hp = p.H + 2 * pad, Wp = p.W + 2 * pad, HW = p.H * p.W;
    const unsigned ntn = (unsigned)(p.Cout / BN);
    const unsigned tmi = blockIdx.x / ntn, tni = blockIdx.x % ntn;                    // column tiles of one row tile are neighbours (shared A rows)
    const long long m0 = (long long)tmi * BM; const int n0 = (int)tni * BN;
    long long pp0;
    {
        const int n = (int)(m0 / HW), r = (int)(m0 - (long long)n * HW), y = r / p.W, x = r - y * p.W;
        pp0 = ((long long)n * Hp + y) * Wp + x;
    }
    unsigned a_voff[NAI];
#pragma unroll
    for (int i = 0; i < NAI; ++i) {
        const int chunk = wave + 8 * i, row = chunk * 16 + lane / 4, pc = lane % 4, lc = pc ^ ((row >> 2) & 3);
        long long m = m0 + row; if (m >= p.M) m = m0;
        const int n = (int)(m / HW), r = (int)(m - (long long)n * HW), y = r / p.W, x = r - y * p.W;
        const long long pp = ((long long)n * Hp + y) * Wp + x - pp0;
        a_voff[i] = (unsigned)(pp * ROWB + lc * 16);
    }
    const bool has_b = wave < NBC;
    unsigned b_voff;
    {
        const int row = (has_b ? wave : 0) * 16 + lane / 4, pc = lane % 4, lc = pc ^ ((row >> 2) & 3);
        b_voff = (unsigned)(row * ROWB + lc * 16);
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const int cpt = p.Cin / 64, nkt = p.K * p.K * cpt;
    int i_c = 0, i_tx = 0, i_ty = 0, i_kt = 0;                                        // the next K-tile to issue: kt = (ty K + tx) cpt + c
    auto issue = [&](int stage) {
        const unsigned st = lds0 + (unsigned)(stage * STAGE);
        const unsigned char* ga = p.xp + (long long)i_c * p.xp_ps + (pp0 + (long long)i_ty * Wp + i_tx) * ROWB;
#pragma unroll
        for (int i = 0; i < NAI; ++i) glds16q(ga, a_voff[i], st + (wave + 8 * i) * 1024);
        if (has_b) glds16q(p.wq + ((long long)i_kt * p.Cout + n0) * ROWB, b_voff, st + ABYTES + wave * 1024);
        ++i_kt;
        if (++i_c == cpt) { i_c = 0; if (++i_tx == p.K) { i_tx = 0; ++i_ty; } }
    };
    accx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    issue(0);
    if (nkt > 1) issue(1);
    for (int kt = 0; kt < nkt; ++kt) {
        // in issue order the youngest instructions are those of tile kt + 1: once only they are outstanding, tile kt has landed
        if (kt + 1 < nkt) { if (has_b) wait_vmq<NAI + 1>(); else wait_vmq<NAI>(); }
        else wait_vmq<0>();
        __builtin_amdgcn_s_barrier();                                 // tile kt is in LDS everywhere; every wave is done reading tile kt - 1's stage
        if (kt + 2 < nkt) issue((kt + 2) % NS);
        const unsigned char* st = smem + (kt % NS) * STAGE;
        fp8x32 af[TM], bfr[TN];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const int r = wr * (TM * 32) + tm * 32 + (lane & 31), sw = (r >> 2) & 3, l0 = 2 * (lane >> 5);
            const int4 u0 = *reinterpret_cast<const int4*>(st + r * ROWB + ((l0) ^ sw) * 16);
            const int4 u1 = *reinterpret_cast<const int4*>(st + r * ROWB + ((l0 + 1) ^ sw) * 16);
            af[tm] = fp8x32{u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
        }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int r = wn * 64 + tn * 32 + (lane & 31), sw = (r >> 2) & 3, l0 = 2 * (lane >> 5);
            const int4 u0 = *reinterpret_cast<const int4*>(st + ABYTES + r * ROWB + ((l0) ^ sw) * 16);
            const int4 u1 = *reinterpret_cast<const int4*>(st + ABYTES + r * ROWB + ((l0 + 1) ^ sw) * 16);
            bfr[tn] = fp8x32{u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
                acc[tm][tn] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[tm], bfr[tn], acc[tm][tn], 0, 0, 0, 127, 0, 127);
        __builtin_amdgcn_s_setprio(0);
    }
    // epilogue: each wave parks one 32 x 32 tile at a time in its own patch of the (now free) stage buffers, then a lane owns (row, 8 channels)
    __syncthreads();
    constexpr int LDP = 36;
    float* patch = reinterpret_cast<float*>(smem) + wave * (32 * LDP);
    const int prow0 = lane >> 2, pc8 = (lane & 3) * 8;
    const int Hq = p.H + 2 * p.yq_pad, Wq = p.W + 2 * p.yq_pad;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const long long mt = m0 + wr * (TM * 32) + tm * 32;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
#pragma unroll
            for (int r = 0; r < 16; ++r) patch[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * LDP + (lane & 31)] = acc[tm][tn][r];
            __builtin_amdgcn_wave_barrier();
            const int col8 = n0 + wn * 64 + tn * 32 + pc8;
            float sc[8], bv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { sc[k] = ldexpf(1.f, p.ex + p.ew[col8 + k]); bv[k] = p.bias ? p.bias[col8 + k] : 0.f; }
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const long long m = mt + prow0 + 16 * it;
                if (m < p.M) {
                    const float4 u0 = *reinterpret_cast<const float4*>(&patch[(prow0 + 16 * it) * LDP + pc8]);
                    const float4 u1 = *reinterpret_cast<const float4*>(&patch[(prow0 + 16 * it) * LDP + pc8 + 4]);
                    const float u[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
                    float v[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) { v[k] = fmaf(u[k], sc[k], bv[k]); if (p.relu) v[k] = v[k] > 0.f ? v[k] : 0.f; }
                    if (p.y) {
                        const long long off = m * p.Cout + col8;
                        *reinterpret_cast<float4*>(p.y + off) = make_float4(v[0], v[1], v[2], v[3]);
                        *reinterpret_cast<float4*>(p.y + off + 4) = make_float4(v[4], v[5], v[6], v[7]);
                    }
                    if (p.yq) {
                        const int n = (int)(m / HW), rem = (int)(m - (long long)n * HW), yy = rem / p.W, xx = rem - yy * p.W;
                        const long long q = ((long long)n * Hq + yy + p.yq_pad) * Wq + xx + p.yq_pad;
                        const float is = ldexpf(1.f, -p.yq_exp);
                        uint2 o;
                        o.x = q8x4(v[0] * is, v[1] * is, v[2] * is, v[3] * is);
                        o.y = q8x4(v[4] * is, v[5] * is, v[6] * is, v[7] * is);
                        *reinterpret_cast<uint2*>(p.yq + (long long)(col8 >> 6) * p.yq_ps + q * 64 + (col8 & 63)) = o;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

bool launch_conv_fp8(const Fp8ConvArgs& a, hipStream_t s)
{
    if (a.Cin % 64 || a.Cout % 64 || a.K % 2 == 0 || a.M <= 0) return false;
    const long long ntm = (a.M + 255) / 256;
    if (a.Cout % 128 == 0) {
        const long long nb = ntm * (a.Cout / 128);
        if (nb > 0x7fffffffLL) return false;
        conv_fp8_kernel<128><<<(unsigned)nb, 512, 0, s>>>(a);
    } else {
        const long long nb = ntm * (a.Cout / 64);
        if (nb > 0x7fffffffLL) return false;
        conv_fp8_kernel<64><<<(unsigned)nb, 512, 0, s>>>(a);
    }
    return true;
}

// ---- weights: per-column maximum, exponent, planes ------------------------------------------------------------------------------------
// amax[co] = max |w[k, co]| over the KK Cin rows of HWIO (bits of non-negative floats order like the values: an integer max is order-independent)
__global__ __launch_bounds__(256) void w_fp8_amax_kernel(const float* __restrict__ w, unsigned* __restrict__ amax, int rows, int Cout, int rows_per)
{
    const int co = blockIdx.x * 256 + threadIdx.x;
    if (co >= Cout) return;
    const int r0 = blockIdx.y * rows_per, r1 = min(rows, r0 + rows_per);
    float mx = 0.f;
    for (int r = r0; r < r1; ++r) mx = fmaxf(mx, fabsf(w[(long long)r * Cout + co]));
    atomicMax(amax + co, __float_as_uint(mx));
}
// ew[co] = E(amax[co]); wq[kt][co][j] = q(w[64 kt + j, co] 2^-ew[co]), 16 bytes per thread
__global__ __launch_bounds__(256) void w_fp8_planes_kernel(const float* __restrict__ w, const unsigned* __restrict__ amax, unsigned char* __restrict__ wq,
                                                           int* __restrict__ ew, int rows, int Cout)
{
    const long long i = blockIdx.x * 256LL + threadIdx.x, total = (long long)rows / 16 * Cout;
    if (i >= total) return;
    const int co = (int)(i % Cout), g = (int)(i / Cout);                       // g = 16-row group: kt = g / 4, bytes (g % 4) * 16 .. + 15 of the row
    const int e = fp8_exponent(__uint_as_float(amax[co]));
    if (g == 0) ew[co] = e;
    const float is = ldexpf(1.f, -e);
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = w[(long long)(g * 16 + j) * Cout + co] * is;
    uint4 o;
    o.x = q8x4(v[0], v[1], v[2], v[3]); o.y = q8x4(v[4], v[5], v[6], v[7]); o.z = q8x4(v[8], v[9], v[10], v[11]); o.w = q8x4(v[12], v[13], v[14], v[15]);
    *reinterpret_cast<uint4*>(wq + ((long long)(g / 4) * Cout + co) * 64 + (g % 4) * 16) = o;
}

void launch_w_to_fp8(const float* w, unsigned char* wq, int* ew, unsigned* amax_scratch, int rows, int Cout, hipStream_t s)      // rows % 64 == 0
{
    hipMemsetAsync(amax_scratch, 0, (size_t)Cout * sizeof(unsigned), s);
    const int slabs = rows >= 4096 ? 64 : (rows >= 512 ? 16 : 1), rows_per = (rows + slabs - 1) / slabs;
    w_fp8_amax_kernel<<<dim3((Cout + 255) / 256, slabs), 256, 0, s>>>(w, amax_scratch, rows, Cout, rows_per);
    const long long total = (long long)rows / 16 * Cout;
    w_fp8_planes_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(w, amax_scratch, wq, ew, rows, Cout);
}

// ---- activations ---------------------------------------------------------------------------------------------------------------------
// x [N][H][W][C] fp32 -> interior of the padded copy (planes of 64 channels), q(x 2^-ex); 16 channels per thread
__global__ __launch_bounds__(256) void f32_to_fp8_padded_kernel(const float* __restrict__ x, unsigned char* __restrict__ xq, int N, int H, int W, int C, int pad,
                                                                long long ps, int ex)
{
    const int c16 = C / 16;
    const long long i = blockIdx.x * 256LL + threadIdx.x, total = (long long)N * H * W * c16;
    if (i >= total) return;
    const long long pix = i / c16; const int c = (int)(i - pix * c16) * 16;
    const int n = (int)(pix / ((long long)H * W)), rem = (int)(pix - (long long)n * H * W), y = rem / W, xx = rem - y * W;
    const long long q = ((long long)n * (H + 2 * pad) + y + pad) * (W + 2 * pad) + xx + pad;
    const float is = ldexpf(1.f, -ex);
    const float4* src = reinterpret_cast<const float4*>(x + pix * C + c);
    const float4 a = src[0], b = src[1], d = src[2], e = src[3];
    uint4 o;
    o.x = q8x4(a.x * is, a.y * is, a.z * is, a.w * is); o.y = q8x4(b.x * is, b.y * is, b.z * is, b.w * is);
    o.z = q8x4(d.x * is, d.y * is, d.z * is, d.w * is); o.w = q8x4(e.x * is, e.y * is, e.z * is, e.w * is);
    *reinterpret_cast<uint4*>(xq + (long long)(c >> 6) * ps + q * 64 + (c & 63)) = o;
}
void launch_f32_to_fp8_padded(const float* x, unsigned char* xq, int N, int H, int W, int C, int pad, long long ps, int ex, hipStream_t s)      // C % 64 == 0
{
    const long long total = (long long)N * H * W * (C / 16);
    if (total > 0) f32_to_fp8_padded_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(x, xq, N, H, W, C, pad, ps, ex);
}

// the border of a padded e4m3 copy (pad rows above / below each image, pad columns left / right of each interior row), every plane: the copies keep their
// storage across shapes and only the border of the current geometry has to be zero -- the producers write every interior position in every pass
__global__ __launch_bounds__(256) void zero_border_fp8_kernel(unsigned char* __restrict__ xq, int planes, long long ps, int N, int H, int W, int pad)
{
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const long long per = 2LL * pad * Wp + 2LL * pad * H, i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= (long long)N * per) return;
    const int n = (int)(i / per); long long j = i - (long long)n * per;
    int y, x;
    if (j < 2LL * pad * Wp) { const int r = (int)(j / Wp); y = r < pad ? r : H + r; x = (int)(j - (long long)r * Wp); }
    else { j -= 2LL * pad * Wp; const int c = (int)(j % (2 * pad)); y = pad + (int)(j / (2 * pad)); x = c < pad ? c : W + c; }
    const long long q = ((long long)n * Hp + y) * Wp + x;
    for (int pl = 0; pl < planes; ++pl) {
        uint4* d = reinterpret_cast<uint4*>(xq + pl * ps + q * 64);
        d[0] = d[1] = d[2] = d[3] = make_uint4(0, 0, 0, 0);
    }
}
void launch_zero_border_fp8(unsigned char* xq, int planes, long long ps, int N, int H, int W, int pad, hipStream_t s)
{
    const long long total = (long long)N * (2LL * pad * (W + 2 * pad) + 2LL * pad * H);
    if (total > 0) zero_border_fp8_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(xq, planes, ps, N, H, W, pad);
}

// 2x2 max-pool of a ReLU output held as a padded e4m3 copy (pad 1, map H x W): non-negative e4m3 codes order like their values, so the pool is a byte max,
// written into the consumer's padded copy (pad ypad, map H/2 x W/2).  Both copies carry the consumer's exponent.  16 channels per thread.
__global__ __launch_bounds__(256) void maxpool_fp8_kernel(const unsigned char* __restrict__ xq, long long xps, unsigned char* __restrict__ yq, long long yps,
                                                          int N, int H, int W, int C, int ypad)
{
    const int Ho = H / 2, Wo = W / 2, c16 = C / 16;
    const long long i = blockIdx.x * 256LL + threadIdx.x, total = (long long)N * Ho * Wo * c16;
    if (i >= total) return;
    const long long pix = i / c16; const int c = (int)(i - pix * c16) * 16;
    const int n = (int)(pix / ((long long)Ho * Wo)), rem = (int)(pix - (long long)n * Ho * Wo), y = rem / Wo, x = rem - y * Wo;
    const unsigned char* src = xq + (long long)(c >> 6) * xps + (c & 63);
    const long long q00 = ((long long)n * (H + 2) + 2 * y + 1) * (W + 2) + 2 * x + 1;
    const uint4 a = *reinterpret_cast<const uint4*>(src + q00 * 64), b = *reinterpret_cast<const uint4*>(src + (q00 + 1) * 64);
    const uint4 d = *reinterpret_cast<const uint4*>(src + (q00 + W + 2) * 64), e = *reinterpret_cast<const uint4*>(src + (q00 + W + 3) * 64);
    auto bmax = [](unsigned u, unsigned v) {
        unsigned r = 0;
#pragma unroll
        for (int k = 0; k < 32; k += 8) r |= max((u >> k) & 255u, (v >> k) & 255u) << k;
        return r;
    };
    uint4 o;
    o.x = bmax(bmax(a.x, b.x), bmax(d.x, e.x)); o.y = bmax(bmax(a.y, b.y), bmax(d.y, e.y));
    o.z = bmax(bmax(a.z, b.z), bmax(d.z, e.z)); o.w = bmax(bmax(a.w, b.w), bmax(d.w, e.w));
    const long long qo = ((long long)n * (Ho + 2 * ypad) + y + ypad) * (Wo + 2 * ypad) + x + ypad;
    *reinterpret_cast<uint4*>(yq + (long long)(c >> 6) * yps + qo * 64 + (c & 63)) = o;
}
void launch_maxpool_fp8(const unsigned char* xq, long long xps, unsigned char* yq, long long yps, int N, int H, int W, int C, int ypad, hipStream_t s)
{
    const long long total = (long long)N * (H / 2) * (W / 2) * (C / 16);
    if (total > 0) maxpool_fp8_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(xq, xps, yq, yps, N, H, W, C, ypad);
}

// calibration: *amax = max(*amax, max |x|) -- an integer max over the bits of non-negative floats, independent of block and lane order (NaNs ignored)
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, long long n, unsigned* __restrict__ amax)
{
    float mx = 0.f;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float a = fabsf(x[i]);
        if (a > mx) mx = a;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(amax, __float_as_uint(mx));
}
void launch_amax(const float* x, long long n, unsigned* amax, hipStream_t s)
{
    long long blocks = (n + 255) / 256; if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
    amax_kernel<<<(unsigned)blocks, 256, 0, s>>>(x, n, amax);
}

}  // namespace fcn8s
