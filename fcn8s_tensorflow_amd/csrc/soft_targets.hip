// Soft-target (distillation) term of the training loss (fcn8s_set_soft_targets, fcn8s_bind_soft_targets; the definition is in fcn8s_hip.h):
//   soft_targets_kernel         one pass over the slots of the logits: kd_p per pixel, dlogits += coef (s - q), per-block partial sums of kd_p and
//                               of the gradient's columns
//   soft_targets_reduce_kernel  one block: the partials summed in a fixed order into the loss, the term slot and the last bias's column sums
//
// Access shape: the tile scheme of temperature.hip, restated here so that temperature.hip and its object stay byte for byte what they were.  A block
// of 256 threads takes a tile of 256 consecutive SLOTS per trip (a slot is a pixel in the plain [npix, C] layout, a place of the blocked layout
// otherwise; lov_slot_pixel's rule is restated as st_slot_pixel).  The tile's 256 C floats of logits and of dlogits are contiguous in slot order in
// both layouts and move with lane-contiguous loads and stores, 16 bytes per lane when the pointers allow it (they always do inside the model: C is
// a multiple of 4 and the arena is aligned), else 4.  The logits land in an LDS image [256][S], S = C if C / 4 is odd, else C + 4 (ds_read_b128
// without conflicts; S = 20 at C = 20); on the 4-byte path S = C if C is odd, else C + 1.  The target rows of the tile's pixels land in a second image
// of the same stride: in the plain layout they are one contiguous run of 256 K floats when row_stride == K; in the blocked layout eight
// consecutive slots are eight consecutive pixels of an image row, so the rows come in contiguous runs of 8 K floats.  They move 16 bytes per lane
// when the pointer is 16-byte aligned and K and row_stride are multiples of 4, else 4 bytes per lane (K = 19 in rows of 19 or 20).
//
// A thread owns row t of both images.  It overwrites its target row by the gradient contribution coef (s_c - q_c) (zeros for the columns >= K, for a
// slot outside the image, for a pixel outside U), and the block then drains dlogits the way it was loaded: every lane adds the image's 16 bytes to the
// 16 bytes of dlogits it holds and stores them where they came from.  dlogits is never staged in LDS.  The columns of the contribution image are
// summed by wave w over rows 64 w .. 64 w + 63, lane = column, the four waves in order; lane c of wave 0 carries column c's running sum over the
// block's tiles.
//
// With C == 20 (the template parameter CT) the next tile's logits, dlogits and -- when K == 20 and the targets take the 16-byte path (TPRE) -- target
// rows are issued into registers before the current tile is worked on; the slot -> pixel map of the next tile is kept in a double-buffered LDS array
// so that a lane can address the target rows of the slots its pieces fall into.  The other shapes fill the images from global memory behind one
// more barrier (correct, not tuned).
//
// Grid: as many blocks as are resident at once (the occupancy the runtime reports for the variant, times 256 CUs; at C = 20 the registers of the
// prefetch allow two blocks per CU), at most 1024 and at most one per tile, so that every block trips over the same number of tiles.
//
// Arithmetic: fp32, expf and logf, classes summed in order, no product contracted into a sum (the header's definition, literally).  kd_p is added to a
// per-thread double, the block's 256 sums are reduced by a shuffle tree and the four waves in order, the blocks' partials by the reduce kernel in a
// fixed order: no float atomics anywhere, two runs give the same bits.
#include "fcn8s_internal.h"
#include <cfloat>
#include <cmath>

namespace fcn8s {
namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_MAX_BLOCKS = 1024;
constexpr int ST_MAX_C = 64;                         // d_lastbias holds 64 columns

__host__ __device__ constexpr int st_vec_stride(int C) { return (C / 4) & 1 ? C : C + 4; }

// slot -> pixel of a (possibly blocked) logits tensor, as lovasz.hip's lov_slot_pixel; -1: the slot lies outside the image
static __device__ __forceinline__ long long st_slot_pixel(long long slot, const PixMap& m)
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

struct StArgs {
    const float* z; float* d; const float* probs; const uint8_t* labels;
    PixMap pm;
    long long nslot, npix, stride;                  // stride: floats between two target rows
    int C, K, S;                                    // S: row stride of the LDS images in floats
    int zvec, tvec, all;                            // 16-byte path of logits / dlogits, of the targets; U = every pixel
    float beta, coef;                               // 1 / T; lambda (T / P)
    double* losspart; float* colpart;               // [blocks], [blocks][ST_MAX_C]
};

// what a thread holds of a tile before it is worked on
template <int NV, bool TPRE>
struct StIn {
    float4 zv[NV > 0 ? NV : 1], dv[NV > 0 ? NV : 1], tv[TPRE ? NV : 1];
    long long pix;                                  // the pixel of slot g0 + t (-1: outside the image or behind the last slot)
    unsigned int lab;
};

// the own slot's pixel and label of tile `tile`; the pixel also goes to pixs[t] for the lanes that load this slot's target row
static __device__ __forceinline__ void st_own(const StArgs& a, long long tile, int t, long long* pixs, long long& pix, unsigned int& lab)
{
    const long long slot = tile * ST_THREADS + t;
    pix = slot < a.nslot ? st_slot_pixel(slot, a.pm) : -1;
    pixs[t] = pix;
    lab = pix >= 0 ? a.labels[pix] : 255u;
}

// (CT path) the tile's pieces of logits, dlogits and target rows into registers; pixs = the tile's slot -> pixel map (visible to the block)
template <int NV, bool TPRE>
static __device__ __forceinline__ void st_load(const StArgs& a, long long tile, int t, const long long* pixs, StIn<NV, TPRE>& in)
{
    const long long g0 = tile * ST_THREADS;
    const long long left = a.nslot - g0;
    const int npx = left < ST_THREADS ? (int)left : ST_THREADS;
    const int nvec = npx * NV;
    const float4* zs = reinterpret_cast<const float4*>(a.z + g0 * (NV * 4));
    const float4* ds = reinterpret_cast<const float4*>(a.d + g0 * (NV * 4));
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = t + k * ST_THREADS;
        const bool in_tile = i < nvec;
        in.zv[k] = in_tile ? zs[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        in.dv[k] = in_tile ? ds[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (TPRE) {                                                                             // K == C == 4 NV: a piece never crosses a row
            constexpr int CD = NV > 0 ? NV * 4 : 1;
            const int f = i * 4, px = f / CD, c = f - px * CD;
            const long long pix = in_tile ? pixs[px] : -1;
            in.tv[k] = pix >= 0 ? *reinterpret_cast<const float4*>(a.probs + pix * a.stride + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

// the tile's npx rows of C floats at src into the image [ST_THREADS][S]
static __device__ __forceinline__ void st_fill_rows(float* img, const float* src, int npx, int C, int S, int vec, int t)
{
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const int nvec = npx * (C / 4);
        for (int i = t; i < nvec; i += ST_THREADS) {
            const int f = i * 4, px = f / C, c = f - px * C;
            *reinterpret_cast<float4*>(img + px * S + c) = s4[i];
        }
    } else {
        const int nfl = npx * C;
        for (int i = t; i < nfl; i += ST_THREADS) {
            const int px = i / C, c = i - px * C;
            img[px * S + c] = src[i];
        }
    }
}

// the target rows of the tile's pixels into columns 0 .. K - 1 of the image (rows of slots without a pixel are left alone: their owner zeroes them)
static __device__ __forceinline__ void st_fill_targets(float* img, const StArgs& a, const long long* pixs, int npx, int t)
{
    const int K = a.K, S = a.S;
    if (a.tvec) {
        const int nvec = npx * (K / 4);
        for (int i = t; i < nvec; i += ST_THREADS) {
            const int f = i * 4, px = f / K, c = f - px * K;
            const long long pix = pixs[px];
            if (pix >= 0) *reinterpret_cast<float4*>(img + px * S + c) = *reinterpret_cast<const float4*>(a.probs + pix * a.stride + c);
        }
    } else {
        const int nfl = npx * K;
        for (int i = t; i < nfl; i += ST_THREADS) {
            const int px = i / K, c = i - px * K;
            const long long pix = pixs[px];
            if (pix >= 0) img[px * S + c] = a.probs[pix * a.stride + c];
        }
    }
}

// One pixel of U: z[0 .. n) its logits, w[0 .. n) its target row (columns >= K hold anything); on return w = coef (s - q) for c < K, 0 for c >= K.
// Returns kd_p.  n = CT (z and w are register arrays, the loops unroll) or C (z and w are the thread's rows of the images).
template <int CT>
static __device__ __forceinline__ float st_pixel(float* z, float* w, int C, int K, float beta, float coef)
{
#pragma clang fp contract(off)
    const int n = CT > 0 ? CT : C;
    bool fin = true;
    float ml = -INFINITY, mz = -INFINITY;
#pragma unroll
    for (int c = 0; c < n; ++c) if (c < K) {
        const float p = w[c];
        fin = fin && isfinite(p);                                                               // tested on p: fmaxf hides a NaN
        const float l = logf(fmaxf(p, FLT_MIN));
        w[c] = l;
        ml = fmaxf(ml, l);
        mz = fmaxf(mz, z[c]);
    }
    float Sq = 0.f, Ss = 0.f;
    float ea[CT > 0 ? CT : 1], eb[CT > 0 ? CT : 1];                                             // CT: the exponentials are kept; else taken again below
#pragma unroll
    for (int c = 0; c < n; ++c) if (c < K) {
        const float av = beta * (w[c] - ml), bv = beta * (z[c] - mz);
        w[c] = av; z[c] = bv;
        const float eav = expf(av), ebv = expf(bv);
        if (CT > 0) { ea[c] = eav; eb[c] = ebv; }
        Sq = Sq + eav;
        Ss = Ss + ebv;
    }
    const float lSq = logf(Sq), lSs = logf(Ss);
    const float qnan = __builtin_nanf("");
    float kd = 0.f;
#pragma unroll
    for (int c = 0; c < n; ++c) {
        if (c < K) {
            const float av = w[c], bv = z[c];
            const float q = (CT > 0 ? ea[c] : expf(av)) / Sq, s = (CT > 0 ? eb[c] : expf(bv)) / Ss;
            const float lq = av - lSq, ls = bv - lSs;
            const float term = q * (lq - ls);
            kd = kd + term;
            const float g = coef * (s - q);
            w[c] = fin ? g : qnan;
        } else {
            w[c] = 0.f;
        }
    }
    return fin ? kd : qnan;
}

// grid: blocks (<= tiles), block: ST_THREADS.  CT: C as a compile-time constant (next-tile loads in registers; needs the 16-byte path), 0 = a.C;
// TPRE: the target rows are among those loads (K == CT, 16-byte path)
template <int CT, bool TPRE>
__global__ __launch_bounds__(ST_THREADS) void soft_targets_kernel(const StArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long st_lds[];
    constexpr int NV = CT / 4, CD = CT > 0 ? CT : 1;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int C = CT > 0 ? CT : a.C, S = CT > 0 ? st_vec_stride(CT) : a.S, K = a.K;
    long long* pixs = reinterpret_cast<long long*>(st_lds);                                     // [2][ST_THREADS]
    double* red = reinterpret_cast<double*>(pixs + 2 * ST_THREADS);                             // [8]
    float* colred = reinterpret_cast<float*>(red + 8);                                          // [4][ST_MAX_C]
    float* zimg = colred + 4 * ST_MAX_C;                                                        // [ST_THREADS][S]: every offset a multiple of 16 bytes
    float* timg = zimg + ST_THREADS * S;                                                        // [ST_THREADS][S]

    const long long tiles = (a.nslot + ST_THREADS - 1) / ST_THREADS;
    double acc = 0.0;
    float colrun = 0.f;                                                                         // wave 0, lane c: column c over the block's tiles
    StIn<NV, TPRE> in;
    int buf = 0;
    if ((long long)blockIdx.x < tiles) {
        st_own(a, blockIdx.x, t, pixs, in.pix, in.lab);
        if (CT > 0) {
            if (TPRE) __syncthreads();
            st_load<NV, TPRE>(a, blockIdx.x, t, pixs, in);
        }
    }
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long g0 = tile * ST_THREADS;
        const long long left = a.nslot - g0;
        const int npx = left < ST_THREADS ? (int)left : ST_THREADS;
        const long long* pcur = pixs + buf * ST_THREADS;
        long long* pnext = pixs + (buf ^ 1) * ST_THREADS;
        const long long mypix = in.pix;
        const unsigned int mylab = in.lab;
        float4 dcur[NV > 0 ? NV : 1];

        // ---- the images of this tile
        if (CT > 0) {
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int f = (t + k * ST_THREADS) * 4, px = f / CD, c = f - px * CD;           // px < 256 for every k < NV
                *reinterpret_cast<float4*>(zimg + px * S + c) = in.zv[k];
                if (TPRE) *reinterpret_cast<float4*>(timg + px * S + c) = in.tv[k];
                dcur[k] = in.dv[k];
            }
            if (!TPRE) { __syncthreads(); st_fill_targets(timg, a, pcur, npx, t); }            // (pcur is visible behind the barrier)
        } else {
            st_fill_rows(zimg, a.z + g0 * C, npx, C, S, a.zvec, t);
            __syncthreads();
            st_fill_targets(timg, a, pcur, npx, t);
        }
        // ---- the next tile's map, then its loads: in flight while this tile is worked on
        const long long next = tile + gridDim.x;
        if (next < tiles) st_own(a, next, t, pnext, in.pix, in.lab);
        __syncthreads();
        if (CT > 0 && next < tiles) st_load<NV, TPRE>(a, next, t, pnext, in);

        // ---- the own row
        {
            float* zr = zimg + t * S;
            float* wr = timg + t * S;
            const bool part = mypix >= 0 && (a.all || mylab < (unsigned int)C);
            if (CT > 0) {
                float zreg[CT > 0 ? CT : 1], wreg[CT > 0 ? CT : 1];
                if (part) {
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        const float4 zq = reinterpret_cast<const float4*>(zr)[i], wq = reinterpret_cast<const float4*>(wr)[i];
                        zreg[4 * i] = zq.x; zreg[4 * i + 1] = zq.y; zreg[4 * i + 2] = zq.z; zreg[4 * i + 3] = zq.w;
                        wreg[4 * i] = wq.x; wreg[4 * i + 1] = wq.y; wreg[4 * i + 2] = wq.z; wreg[4 * i + 3] = wq.w;
                    }
                    acc += (double)st_pixel<CT>(zreg, wreg, C, K, a.beta, a.coef);
                } else {
#pragma unroll
                    for (int i = 0; i < (CT > 0 ? CT : 1); ++i) wreg[i] = 0.f;
                }
#pragma unroll
                for (int i = 0; i < NV; ++i)
                    reinterpret_cast<float4*>(wr)[i] = make_float4(wreg[4 * i], wreg[4 * i + 1], wreg[4 * i + 2], wreg[4 * i + 3]);
            } else if (part) {
                acc += (double)st_pixel<0>(zr, wr, C, K, a.beta, a.coef);
            } else {
                for (int c = 0; c < C; ++c) wr[c] = 0.f;
            }
        }
        __syncthreads();

        // ---- drain dlogits the way it was loaded; the column sums of the contribution image
        if (CT > 0) {
            float4* dst = reinterpret_cast<float4*>(a.d + g0 * C);
            const int nvec = npx * NV;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int i = t + k * ST_THREADS;
                const int f = i * 4, px = f / CD, c = f - px * CD;
                const float4 g = *reinterpret_cast<const float4*>(timg + px * S + c);
                if (i < nvec) dst[i] = make_float4(dcur[k].x + g.x, dcur[k].y + g.y, dcur[k].z + g.z, dcur[k].w + g.w);
            }
        } else if (a.zvec) {
            float4* dst = reinterpret_cast<float4*>(a.d + g0 * C);
            const int nvec = npx * (C / 4);
            for (int i = t; i < nvec; i += ST_THREADS) {
                const int f = i * 4, px = f / C, c = f - px * C;
                const float4 g = *reinterpret_cast<const float4*>(timg + px * S + c);
                const float4 o = dst[i];
                dst[i] = make_float4(o.x + g.x, o.y + g.y, o.z + g.z, o.w + g.w);
            }
        } else {
            float* dst = a.d + g0 * C;
            const int nfl = npx * C;
            for (int i = t; i < nfl; i += ST_THREADS) {
                const int px = i / C, c = i - px * C;
                dst[i] = dst[i] + timg[px * S + c];
            }
        }
        {
            float v = 0.f;
            if (lane < K) {
                const float* col = timg + (wave * 64) * S + lane;
                for (int r = 0; r < 64; ++r) v = v + col[r * S];
            }
            colred[wave * ST_MAX_C + lane] = v;
        }
        __syncthreads();                                                                        // the images are free for the next tile
        if (wave == 0) colrun = colrun + (((colred[lane] + colred[ST_MAX_C + lane]) + colred[2 * ST_MAX_C + lane]) + colred[3 * ST_MAX_C + lane]);
        buf ^= 1;
    }

    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (t == 0) a.losspart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    if (wave == 0) a.colpart[(size_t)blockIdx.x * ST_MAX_C + lane] = colrun;
}

// one block of 256: the blocks' partials in a fixed order.  kd = (T^2 / P) sum kd_p -> term[0]; loss[0] += lambda kd; lastbias[c] += column c's sum
__global__ __launch_bounds__(ST_THREADS) void soft_targets_reduce_kernel(const double* losspart, const float* colpart, int nblocks, int K, double tt_over_p,
                                                                         float lambda, float* loss, float* term, float* lastbias)
{
    __shared__ double sh[4];
    __shared__ float cs[4][ST_MAX_C];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double v = 0.0;
    for (int b = t; b < nblocks; b += ST_THREADS) v += losspart[b];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) sh[wave] = v;
    float c = 0.f;
    if (lane < K) for (int b = wave; b < nblocks; b += 4) c = c + colpart[(size_t)b * ST_MAX_C + lane];
    cs[wave][lane] = c;
    __syncthreads();
    if (t == 0) {
#pragma clang fp contract(off)
        const float kd = (float)((((sh[0] + sh[1]) + sh[2]) + sh[3]) * tt_over_p);
        term[0] = kd;
        const float add = lambda * kd;
        loss[0] = loss[0] + add;
    }
    if (t < K) lastbias[t] = lastbias[t] + (((cs[0][t] + cs[1][t]) + cs[2][t]) + cs[3][t]);
}

size_t st_lds_bytes(int S) { return (size_t)2 * ST_THREADS * 8 + 8 * 8 + (size_t)4 * ST_MAX_C * 4 + (size_t)2 * ST_THREADS * S * 4; }

template <int CT, bool TPRE>
int st_launch(const StArgs& a, int blocks, size_t lds, hipStream_t s)          // -> the blocks launched (0: refused)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&soft_targets_kernel<CT, TPRE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "soft_targets: %zu bytes of LDS refused (%s)", lds, hipGetErrorString(e)); return 0; }
    }
    // no more blocks than are resident at once, so that every block trips over the same number of tiles (256 CUs; the registers, not the LDS, decide)
    static int resident = 0; static size_t resident_lds = 0;
    if (!resident || resident_lds != lds) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(&soft_targets_kernel<CT, TPRE>), ST_THREADS, lds) != hipSuccess || n < 1) { n = 1; (void)hipGetLastError(); }
        resident = n; resident_lds = lds;
    }
    if (blocks > 256 * resident) blocks = 256 * resident;
    hipLaunchKernelGGL((soft_targets_kernel<CT, TPRE>), dim3(blocks), dim3(ST_THREADS), lds, s, a);
    return blocks;
}

}  // namespace

size_t soft_targets_scratch_bytes() { return (size_t)ST_MAX_BLOCKS * (8 + ST_MAX_C * 4); }

double soft_targets_bytes(long long npix, int C, int K) { return (double)npix * (4.0 * C + 4.0 * K + 1.0 + 8.0 * C); }

void launch_soft_targets(const float* logits, float* dlogits, const float* probs, const uint8_t* labels, const PixMap* map, int N, long long npix, int C,
                         int K, long long row_stride, float lambda, float temperature, int all_pixels, char* ws, float* loss, float* term,
                         float* lastbias, hipStream_t s)
{
    if (C < 1 || C > ST_MAX_C || K < 1 || K > C || row_stride < K) { defer_error(FCN8S_ERR_BAD_ARG, "soft_targets: C = %d, K = %d, row stride %lld", C, K, row_stride); return; }
    StArgs a = {};
    a.z = logits; a.d = dlogits; a.probs = probs; a.labels = labels;
    a.pm = map ? *map : PixMap{0, 0, 0, 0, 0, 0};
    a.npix = npix; a.nslot = pixmap_slots(a.pm, npix, N); a.stride = row_stride;
    a.C = C; a.K = K; a.all = all_pixels;
    a.beta = 1.f / temperature;
    a.coef = lambda * (temperature / (float)npix);
    a.zvec = (((uintptr_t)logits | (uintptr_t)dlogits) & 15) == 0 && C % 4 == 0;
    a.tvec = ((uintptr_t)probs & 15) == 0 && K % 4 == 0 && row_stride % 4 == 0;
    a.S = a.zvec ? st_vec_stride(C) : (C & 1 ? C : C + 1);
    a.losspart = reinterpret_cast<double*>(ws);
    a.colpart = reinterpret_cast<float*>(ws + (size_t)ST_MAX_BLOCKS * 8);
    const size_t lds = st_lds_bytes(a.S);
    const long long tiles = (a.nslot + ST_THREADS - 1) / ST_THREADS;
    long long per_cu = (long long)(160 * 1024 / lds);                                           // blocks resident at once: 256 CUs, 160 KB of LDS each
    per_cu = per_cu > 4 ? 4 : (per_cu < 1 ? 1 : per_cu);
    long long blocks = tiles < ST_MAX_BLOCKS ? tiles : ST_MAX_BLOCKS;
    if (blocks > 256 * per_cu) blocks = 256 * per_cu;
    if (blocks < 1) blocks = 1;
    int launched;
    if (a.zvec && C == 20 && a.tvec && K == 20) launched = st_launch<20, true>(a, (int)blocks, lds, s);
    else if (a.zvec && C == 20) launched = st_launch<20, false>(a, (int)blocks, lds, s);
    else launched = st_launch<0, false>(a, (int)blocks, lds, s);
    if (!launched) return;
    hipLaunchKernelGGL(soft_targets_reduce_kernel, dim3(1), dim3(ST_THREADS), 0, s, (const double*)a.losspart, (const float*)a.colpart, launched, K,
                       (double)temperature * (double)temperature / (double)npix, lambda, loss, term, lastbias);
}

}  // namespace fcn8s
