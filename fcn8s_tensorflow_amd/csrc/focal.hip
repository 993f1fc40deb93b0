// Focal loss of the training objective (fcn8s_set_focal, fcn8s_op_focal_xent; the definition is in fcn8s_hip.h):
//   focal_xent_kernel         one pass over the slots of the logits: L_p = w_p (f l) per valid pixel, dlogits = the cross-entropy's gradient row times the
//                             per-pixel scalar c_p (STORED: this kernel stands where the cross-entropy's stands), per-block partial sums of the loss, of
//                             the valid pixels and of the gradient's columns
//   focal_xent_reduce_kernel  one block of 1024: the partials summed in a fixed order into the loss (or its double sum), |V| and the last bias's column sums
//
// Access shape: the tile scheme of entropy_min.hip, restated here so that entropy_min.hip, soft_targets.hip, elementwise.hip and their objects stay
// byte for byte what they were.  A block of 256 threads takes a tile of 256 consecutive SLOTS per trip (a slot is a pixel in the plain [npix, C]
// layout, a place of the blocked layout otherwise; lov_slot_pixel's rule is restated as fo_slot_pixel).  The tile's 256 C floats of logits and of
// dlogits are contiguous in slot order in both layouts and move with lane-contiguous loads and stores, 16 bytes per lane when the pointers allow it
// (they always do inside the model: C is a multiple of 4 and the arena is aligned), else 4.  The logits land in ONE LDS image [256][S], S = C if
// C / 4 is odd, else C + 4 (ds_read_b128 without conflicts; S = 20 at C = 20); on the 4-byte path S = C if C is odd, else C + 1.  The class weights
// (64 floats) and the 256-entry table lie in LDS in front of the image.
//
// A thread owns row t of the image.  It overwrites its row by the gradient row -- by zeros for a slot outside the image and for an ignored pixel --
// and the block then drains the image to dlogits the way the logits came in: every lane stores the image's 16 bytes where the logits' 16 bytes came
// from.  Without dlogits (the op's loss-only call) nothing is stored.  The columns of the gradient image are summed by wave w over rows 64 w ..
// 64 w + 63, lane = column, the four waves in order; lane c of wave 0 carries column c's running sum over the block's tiles.
//
// With C == 20 (the template parameter CT) the next tile's logits, labels and codes are issued into registers before the current tile is worked on.
// The other shapes fill the image from global memory behind one more barrier (correct, not tuned).
//
// Grid: as many blocks as are resident at once (the occupancy the runtime reports for the variant, times 256 CUs), at most 1024 and at most one per
// tile, so that every block trips over the same number of tiles.
//
// Arithmetic: fp32, expf and logf, classes summed in order, no product contracted into a sum (the header's definition, literally).  w_p (f l) is added
// to a per-thread double, the block's 256 sums are reduced by a shuffle tree and the four waves in order, the blocks' partials by the reduce kernel in
// a fixed order: no float atomics, no ticket, no fence, every loop bounded; two runs give the same bits, whatever the `deterministic` option says.
#include "fcn8s_internal.h"
#include <cfloat>
#include <cmath>

namespace fcn8s {
namespace {

constexpr int FO_THREADS = 256;
constexpr int FO_MAX_BLOCKS = 1024;
constexpr int FO_RED_THREADS = 1024;                   // the reduce kernel's one block
constexpr int FO_MAX_C = 64;                           // d_lastbias holds 64 columns

__host__ __device__ constexpr int fo_vec_stride(int C) { return (C / 4) & 1 ? C : C + 4; }

// slot -> pixel of a (possibly blocked) logits tensor, as lovasz.hip's lov_slot_pixel; -1: the slot lies outside the image
static __device__ __forceinline__ long long fo_slot_pixel(long long slot, const PixMap& m)
{
    if (!m.blocked) return slot;
    const int S = m.S;
    const int rx = (int)(slot % S); long long t = slot / S;
    const int r = (int)(t % S); t /= S;
    const int qx = (int)(t % m.QW); t /= m.QW;
    const int q = (int)(t % m.QH); const long long n = t / m.QH;
    const int oy = q * S - S / 2 + r, ox = qx * S - S / 2 + rx;
    if ((unsigned)oy >= (unsigned)m.H || (unsigned)ox >= (unsigned)m.W) return -1;
    return (n * m.H + oy) * m.W + ox;
}

struct FoArgs {
    const float* z; float* d; const uint8_t* labels;   // d may be null: the loss and the column sums only
    const float* cw; const uint8_t* codes; const float* ptab;   // null: all weights 1; codes and ptab both set or both null
    PixMap pm;
    long long nslot;
    int C, S;                                       // S: row stride of the LDS image in floats
    int zvec;                                       // 16-byte path of logits / dlogits
    float gamma, gscale;                            // gscale = ce_weight / P
    double* losspart; unsigned long long* validpart; float* colpart;    // [blocks], [blocks], [blocks][FO_MAX_C]
};

// what a thread holds of a tile before it is worked on
template <int NV>
struct FoIn {
    float4 zv[NV > 0 ? NV : 1];
    int lab;                                        // the label of slot g0 + t; -1: no valid pixel there
    int code;
};

// the label (and the distance code) of the own slot of tile `tile`; lab = -1 for a slot outside the image and for an ignored pixel
static __device__ __forceinline__ void fo_own(const FoArgs& a, long long tile, int t, int& lab, int& code)
{
    const long long slot = tile * FO_THREADS + t;
    const long long pix = slot < a.nslot ? fo_slot_pixel(slot, a.pm) : -1;
    lab = -1; code = 0;
    if (pix < 0) return;
    const int y = a.labels[pix];
    if (y >= a.C) return;
    lab = y;
    if (a.codes) code = a.codes[pix];
}

// (CT path) the tile's pieces of the logits into registers
template <int NV>
static __device__ __forceinline__ void fo_load(const FoArgs& a, long long tile, int t, FoIn<NV>& in)
{
    const long long g0 = tile * FO_THREADS;
    const long long left = a.nslot - g0;
    const int npx = left < FO_THREADS ? (int)left : FO_THREADS;
    const int nvec = npx * NV;
    const float4* zs = reinterpret_cast<const float4*>(a.z + g0 * (NV * 4));
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = t + k * FO_THREADS;
        in.zv[k] = i < nvec ? zs[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// the tile's npx rows of C floats at src into the image [FO_THREADS][S]
static __device__ __forceinline__ void fo_fill_rows(float* img, const float* src, int npx, int C, int S, int vec, int t)
{
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const int nvec = npx * (C / 4);
        for (int i = t; i < nvec; i += FO_THREADS) {
            const int f = i * 4, px = f / C, c = f - px * C;
            *reinterpret_cast<float4*>(img + px * S + c) = s4[i];
        }
    } else {
        const int nfl = npx * C;
        for (int i = t; i < nfl; i += FO_THREADS) {
            const int px = i / C, c = i - px * C;
            img[px * S + c] = src[i];
        }
    }
}

// One valid pixel: z[0 .. n) its logits, y its label, w its weight w_p; on return z = the gradient row.  Returns f l (the caller weights it).
// n = CT (z is a register array, the loops unroll, the exponentials are kept) or C (z is the thread's row of the image, the exponentials are
// taken again: expf of the same float is the same float).
template <int CT>
static __device__ __forceinline__ float fo_pixel(float* z, int C, int y, float w, float gamma, float gscale)
{
#pragma clang fp contract(off)
    const int n = CT > 0 ? CT : C;
    float mz = z[0];
#pragma unroll
    for (int c = 1; c < n; ++c) mz = fmaxf(mz, z[c]);
    float S = 0.f, R = 0.f, zy = 0.f, ey = 0.f;
    float e[CT > 0 ? CT : 1];
#pragma unroll
    for (int c = 0; c < n; ++c) {
        const float ec = expf(z[c] - mz);
        if (CT > 0) e[c] = ec;
        S = S + ec;
        if (c == y) { zy = z[c]; ey = ec; } else R = R + ec;
    }
    const float l = (mz + logf(S)) - zy;
    const float u = R / S, sy = ey / S;
    float f = 0.f, av = 0.f;
    if (u != 0.f) {
        const float t = expf((gamma - 1.f) * logf(fmaxf(u, FLT_MIN)));
        const float lsy = l * sy;
        const float glsy = gamma * lsy;
        f = t * u;
        av = t * (u + glsy);
    }
    const float g = gscale * w;
    const float cp = g * av;
    const float q = cp / S;
    const float cu = cp * u;
#pragma unroll
    for (int c = 0; c < n; ++c) {
        const float ec = CT > 0 ? e[c] : expf(z[c] - mz);
        z[c] = c == y ? -cu : ec * q;
    }
    return f * l;
}

// grid: blocks (<= tiles), block: FO_THREADS.  CT: C as a compile-time constant (next-tile loads in registers; needs the 16-byte path), 0 = a.C
template <int CT>
__global__ __launch_bounds__(FO_THREADS) void focal_xent_kernel(const FoArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long fo_lds[];
    constexpr int NV = CT / 4, CD = CT > 0 ? CT : 1;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int C = CT > 0 ? CT : a.C, S = CT > 0 ? fo_vec_stride(CT) : a.S;
    double* red = reinterpret_cast<double*>(fo_lds);                                            // [4]
    unsigned long long* vred = reinterpret_cast<unsigned long long*>(red + 4);                  // [4]
    float* colred = reinterpret_cast<float*>(vred + 4);                                         // [4][FO_MAX_C]
    float* wsh = colred + 4 * FO_MAX_C;                                                         // [FO_MAX_C]
    float* tab = wsh + FO_MAX_C;                                                                // [256]
    float* img = tab + 256;                                                                     // [FO_THREADS][S]: the offset is a multiple of 16 bytes

    if (t < FO_MAX_C) wsh[t] = a.cw && t < C ? a.cw[t] : 1.f;
    tab[t] = a.ptab ? a.ptab[t] : 1.f;
    // (the first tile's barrier below stands between these stores and their first read)

    const long long tiles = (a.nslot + FO_THREADS - 1) / FO_THREADS;
    double acc = 0.0;
    unsigned long long nvalid = 0;
    float colrun = 0.f;                                                                         // wave 0, lane c: column c over the block's tiles
    FoIn<NV> in;
    in.lab = -1; in.code = 0;
    if ((long long)blockIdx.x < tiles) {
        fo_own(a, blockIdx.x, t, in.lab, in.code);
        if (CT > 0) fo_load<NV>(a, blockIdx.x, t, in);
    }
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long g0 = tile * FO_THREADS;
        const long long left = a.nslot - g0;
        const int npx = left < FO_THREADS ? (int)left : FO_THREADS;
        const int lab = in.lab, code = in.code;

        // ---- the image of this tile
        if (CT > 0) {
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int f = (t + k * FO_THREADS) * 4, px = f / CD, c = f - px * CD;           // px < 256 for every k < NV
                *reinterpret_cast<float4*>(img + px * S + c) = in.zv[k];
            }
        } else {
            fo_fill_rows(img, a.z + g0 * C, npx, C, S, a.zvec, t);
        }
        // ---- the next tile's loads: in flight while this tile is worked on
        const long long next = tile + gridDim.x;
        if (next < tiles) {
            fo_own(a, next, t, in.lab, in.code);
            if (CT > 0) fo_load<NV>(a, next, t, in);
        }
        __syncthreads();

        // ---- the own row
        {
            float* zr = img + t * S;
            const bool part = lab >= 0;
            float w = 1.f;
            if (part) {
#pragma clang fp contract(off)
                w = wsh[lab];
                if (a.ptab) w = w * tab[code];
                ++nvalid;
            }
            if (CT > 0) {
                float zreg[CT > 0 ? CT : 1];
                if (part) {
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        const float4 zq = reinterpret_cast<const float4*>(zr)[i];
                        zreg[4 * i] = zq.x; zreg[4 * i + 1] = zq.y; zreg[4 * i + 2] = zq.z; zreg[4 * i + 3] = zq.w;
                    }
                    const float fl = fo_pixel<CT>(zreg, C, lab, w, a.gamma, a.gscale);
                    acc += (double)w * (double)fl;
                } else {
#pragma unroll
                    for (int i = 0; i < (CT > 0 ? CT : 1); ++i) zreg[i] = 0.f;
                }
#pragma unroll
                for (int i = 0; i < NV; ++i)
                    reinterpret_cast<float4*>(zr)[i] = make_float4(zreg[4 * i], zreg[4 * i + 1], zreg[4 * i + 2], zreg[4 * i + 3]);
            } else if (part) {
                const float fl = fo_pixel<0>(zr, C, lab, w, a.gamma, a.gscale);
                acc += (double)w * (double)fl;
            } else {
                for (int c = 0; c < C; ++c) zr[c] = 0.f;
            }
        }
        __syncthreads();

        // ---- drain the image to dlogits the way the logits were loaded; the column sums of the gradient image
        if (a.d) {
            if (CT > 0) {
                float4* dst = reinterpret_cast<float4*>(a.d + g0 * C);
                const int nvec = npx * NV;
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int i = t + k * FO_THREADS;
                    const int f = i * 4, px = f / CD, c = f - px * CD;
                    if (i < nvec) dst[i] = *reinterpret_cast<const float4*>(img + px * S + c);
                }
            } else if (a.zvec) {
                float4* dst = reinterpret_cast<float4*>(a.d + g0 * C);
                const int nvec = npx * (C / 4);
                for (int i = t; i < nvec; i += FO_THREADS) {
                    const int f = i * 4, px = f / C, c = f - px * C;
                    dst[i] = *reinterpret_cast<const float4*>(img + px * S + c);
                }
            } else {
                float* dst = a.d + g0 * C;
                const int nfl = npx * C;
                for (int i = t; i < nfl; i += FO_THREADS) {
                    const int px = i / C, c = i - px * C;
                    dst[i] = img[px * S + c];
                }
            }
        }
        {
            float v = 0.f;
            if (lane < C) {
                const float* col = img + (wave * 64) * S + lane;
                for (int r = 0; r < 64; ++r) v = v + col[r * S];
            }
            colred[wave * FO_MAX_C + lane] = v;
        }
        __syncthreads();                                                                        // the image is free for the next tile
        if (wave == 0) colrun = colrun + (((colred[lane] + colred[FO_MAX_C + lane]) + colred[2 * FO_MAX_C + lane]) + colred[3 * FO_MAX_C + lane]);
    }

    for (int o = 32; o > 0; o >>= 1) { acc += __shfl_down(acc, o, 64); nvalid += __shfl_down(nvalid, o, 64); }
    if (lane == 0) { red[wave] = acc; vred[wave] = nvalid; }
    __syncthreads();
    if (t == 0) {
        a.losspart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
        a.validpart[blockIdx.x] = ((vred[0] + vred[1]) + vred[2]) + vred[3];
    }
    if (wave == 0) a.colpart[(size_t)blockIdx.x * FO_MAX_C + lane] = colrun;
}

// one block of 1024: the blocks' partials in a fixed order.  With `sum_out` (the model): sum_out[0] = the double sum, which finalize_loss divides by P
// and rounds once; with `loss` (the op): loss[0] = fl(sum / P).  st (may be null): |V| into the loss state fcn8s_get_loss_stats reads.  bias (may be
// null): bias[c] = column c's sum.  Wave w of the 16 sums column `lane` over the blocks w, w + 16, ... in order, eight loads in flight at a time;
// then the 16 waves in order (entropy_min.hip's reduction, which measured a narrower one at 40 us per call).
__global__ __launch_bounds__(FO_RED_THREADS) void focal_xent_reduce_kernel(const double* __restrict__ losspart, const unsigned long long* __restrict__ validpart,
                                                                           const float* __restrict__ colpart, int nblocks, int C, double den, double* sum_out,
                                                                           float* loss, OhemState* st, float* bias)
{
    constexpr int NW = FO_RED_THREADS / 64;
    __shared__ double sh[NW];
    __shared__ unsigned long long vh[NW];
    __shared__ float cs[NW][FO_MAX_C];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double v = 0.0;
    unsigned long long nv = 0;
    for (int b = t; b < nblocks; b += FO_RED_THREADS) { v += losspart[b]; nv += validpart[b]; }
    for (int o = 32; o > 0; o >>= 1) { v += __shfl_down(v, o, 64); nv += __shfl_down(nv, o, 64); }
    if (lane == 0) { sh[wave] = v; vh[wave] = nv; }
    float c = 0.f;
    if (lane < C) {
        int b = wave;
        for (; b + 7 * NW < nblocks; b += 8 * NW) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = colpart[(size_t)(b + j * NW) * FO_MAX_C + lane];
#pragma unroll
            for (int j = 0; j < 8; ++j) c = c + x[j];
        }
        for (; b < nblocks; b += NW) c = c + colpart[(size_t)b * FO_MAX_C + lane];
    }
    cs[wave][lane] = c;
    __syncthreads();
    if (t == 0) {
        double sum = sh[0];
        unsigned long long valid = vh[0];
        for (int w = 1; w < NW; ++w) { sum += sh[w]; valid += vh[w]; }
        if (sum_out) sum_out[0] = sum;
        if (loss) loss[0] = (float)(sum / den);
        if (st) { st->valid = valid; st->ntau = 0; st->kept = valid; st->t = 0.f; }
    }
    if (bias && t < C) {
        float sum = cs[0][t];
        for (int w = 1; w < NW; ++w) sum = sum + cs[w][t];
        bias[t] = sum + 0.f;                                                                    // (+0 for a batch without a valid pixel, not -0)
    }
}

size_t fo_lds_bytes(int S) { return 4 * 8 + 4 * 8 + (size_t)4 * FO_MAX_C * 4 + FO_MAX_C * 4 + 256 * 4 + (size_t)FO_THREADS * S * 4; }

template <int CT>
int fo_launch(const FoArgs& a, int blocks, size_t lds, hipStream_t s)          // -> the blocks launched (0: refused)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&focal_xent_kernel<CT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "focal_xent: %zu bytes of LDS refused (%s)", lds, hipGetErrorString(e)); return 0; }
    }
    // no more blocks than are resident at once, so that every block trips over the same number of tiles (256 CUs; what the runtime reports decides)
    static int resident = 0; static size_t resident_lds = 0;
    if (!resident || resident_lds != lds) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(&focal_xent_kernel<CT>), FO_THREADS, lds) != hipSuccess || n < 1) { n = 1; (void)hipGetLastError(); }
        resident = n; resident_lds = lds;
    }
    if (blocks > 256 * resident) blocks = 256 * resident;
    hipLaunchKernelGGL((focal_xent_kernel<CT>), dim3(blocks), dim3(FO_THREADS), lds, s, a);
    return blocks;
}

}  // namespace

size_t focal_xent_scratch_bytes() { return (size_t)FO_MAX_BLOCKS * (8 + 8 + FO_MAX_C * 4); }

double focal_xent_bytes(long long npix, int C, bool codes) { return (double)npix * (8.0 * C + (codes ? 2.0 : 1.0)); }

void launch_focal_xent(const float* logits, float* dlogits, const uint8_t* labels, const float* cw, const uint8_t* codes, const float* ptab, const PixMap* map,
                       int N, long long npix, int C, float gamma, float gscale, char* ws, double* sum_out, float* loss, OhemState* st, float* bias, hipStream_t s)
{
    if (C < 2 || C > FO_MAX_C || N < 1 || npix < N || !(gamma > 0.f) || !(gamma <= 8.f) || !codes != !ptab) {
        defer_error(FCN8S_ERR_BAD_ARG, "focal_xent: C = %d, N = %d, gamma = %g", C, N, (double)gamma); return;
    }
    FoArgs a = {};
    a.z = logits; a.d = dlogits; a.labels = labels; a.cw = cw; a.codes = codes; a.ptab = ptab;
    a.pm = map ? *map : PixMap{0, 0, 0, 0, 0, 0};
    a.nslot = pixmap_slots(a.pm, npix, N);
    a.C = C; a.gamma = gamma; a.gscale = gscale;
    a.zvec = (((uintptr_t)logits | (uintptr_t)dlogits) & 15) == 0 && C % 4 == 0;                // (null dlogits: the logits alone decide)
    a.S = a.zvec ? fo_vec_stride(C) : (C & 1 ? C : C + 1);
    a.losspart = reinterpret_cast<double*>(ws);
    a.validpart = reinterpret_cast<unsigned long long*>(ws + (size_t)FO_MAX_BLOCKS * 8);
    a.colpart = reinterpret_cast<float*>(ws + (size_t)FO_MAX_BLOCKS * 16);
    const size_t lds = fo_lds_bytes(a.S);
    const long long tiles = (a.nslot + FO_THREADS - 1) / FO_THREADS;
    long long blocks = tiles < FO_MAX_BLOCKS ? tiles : FO_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    const int launched = a.zvec && C == 20 ? fo_launch<20>(a, (int)blocks, lds, s) : fo_launch<0>(a, (int)blocks, lds, s);
    if (!launched) return;
    hipLaunchKernelGGL(focal_xent_reduce_kernel, dim3(1), dim3(FO_RED_THREADS), 0, s, (const double*)a.losspart, (const unsigned long long*)a.validpart,
                       (const float*)a.colpart, launched, C, (double)npix, sum_out, loss, st, bias);
}

}  // namespace fcn8s
