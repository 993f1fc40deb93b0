// Soft-target (distillation) term of the training loss (fcn8s_set_soft_targets, fcn8s_bind_soft_targets; the definition is in fcn8s_hip.h):
//   soft_targets_kernel         one pass over the slots of the logits: kd_p per pixel, dlogits += coef (s - q), per-block partial sums of kd_p and
//                               of the gradient's columns
//   soft_targets_reduce_kernel  one block: the partials summed in a fixed order into the loss, the term slot and the last bias's column sums
//
// The tile frame's pieces are loss_tile.h's; the loop is this file's own, for what the term adds.  The target rows of the tile's pixels land in a second
// image of the same stride, and a thread overwrites its TARGET row by the gradient contribution coef (s_c - q_c) (zeros for the columns >= K, for a slot
// outside the image, for a pixel outside U), which a drain that adds takes to dlogits.  In the plain layout the target rows are one contiguous run of
// 256 K floats when row_stride == K; in the blocked layout eight consecutive slots are eight consecutive pixels of an image row, so the rows come in
// contiguous runs of 8 K floats.  They move 16 bytes per lane when the pointer is 16-byte aligned and K and row_stride are multiples of 4, else 4 bytes
// per lane (K = 19 in rows of 19 or 20).
//
// With C == 20 (CT) and -- when K == 20 and the targets take the 16-byte path (TPRE) -- the target rows are among the next tile's loads into registers;
// the slot -> pixel map of the next tile is kept in a double-buffered LDS array in front of the frame's LDS, so that a lane can address the target rows
// of the slots its pieces fall into, behind one more barrier.  At C = 20 the registers of the prefetch allow two blocks per CU.
//
// Arithmetic: fp32, expf and logf, classes summed in order, no product contracted into a sum (the header's definition, literally).
#include "loss_tile.h"
#include <cfloat>
#include <cmath>

namespace fcn8s {
namespace {

namespace lt = loss_tile;
constexpr int ST_RED_THREADS = 256;                    // the reduce kernel's one block

struct StArgs : lt::Args {
    const float* probs; const uint8_t* labels;
    long long stride;                               // floats between two target rows
    int K;
    int tvec, all;                                  // 16-byte path of the targets; U = every pixel
    float beta, coef;                               // 1 / T; lambda (T / P)
};

// what a thread learns about its own slot of tile `tile`: its pixel (-1: outside the image or behind the last slot) and label; the pixel also goes to
// pixs[t] for the lanes that load this slot's target row
struct StOwn { long long pix; unsigned int lab; };
static __device__ __forceinline__ StOwn st_own(const StArgs& a, long long tile, int t, long long* pixs)
{
    const long long slot = tile * lt::THREADS + t;
    StOwn o;
    o.pix = slot < a.nslot ? slot_pixel(slot, a.pm) : -1;
    pixs[t] = o.pix;
    o.lab = o.pix >= 0 ? a.labels[o.pix] : 255u;
    return o;
}

// (TPRE) the tile's pieces of the target rows into registers; pixs = the tile's slot -> pixel map (visible to the block)
template <int NV>
static __device__ __forceinline__ void st_load_targets(const StArgs& a, long long tile, int t, const long long* pixs, float4* tv)
{
    const int nvec = lt::tile_rows(a.nslot, tile) * NV;
#pragma unroll
    for (int k = 0; k < NV; ++k) {                                                              // K == C == 4 NV: a piece never crosses a row
        constexpr int CD = NV > 0 ? NV * 4 : 1;
        const int i = t + k * lt::THREADS;
        const int f = i * 4, px = f / CD, c = f - px * CD;
        const long long pix = i < nvec ? pixs[px] : -1;
        tv[k] = pix >= 0 ? *reinterpret_cast<const float4*>(a.probs + pix * a.stride + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// the target rows of the tile's pixels into columns 0 .. K - 1 of the image (rows of slots without a pixel are left alone: their owner zeroes them)
static __device__ __forceinline__ void st_fill_targets(float* img, const StArgs& a, const long long* pixs, int npx, int t)
{
    const int K = a.K, S = a.S;
    if (a.tvec) {
        const int nvec = npx * (K / 4);
        for (int i = t; i < nvec; i += lt::THREADS) {
            const int f = i * 4, px = f / K, c = f - px * K;
            const long long pix = pixs[px];
            if (pix >= 0) *reinterpret_cast<float4*>(img + px * S + c) = *reinterpret_cast<const float4*>(a.probs + pix * a.stride + c);
        }
    } else {
        const int nfl = npx * K;
        for (int i = t; i < nfl; i += lt::THREADS) {
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

// grid: blocks (<= tiles), block: lt::THREADS.  CT: C as a compile-time constant (next-tile loads in registers; needs the 16-byte path), 0 = a.C;
// TPRE: the target rows are among those loads (K == CT, 16-byte path)
template <int CT, bool TPRE>
__global__ __launch_bounds__(lt::THREADS) void soft_targets_kernel(const StArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long st_lds[];
    constexpr int NV = CT / 4, CD = CT > 0 ? CT : 1;
    const int t = threadIdx.x, wave = t >> 6;
    const int C = CT > 0 ? CT : a.C, S = CT > 0 ? lt::vec_stride(CT) : a.S, K = a.K;
    long long* pixs = reinterpret_cast<long long*>(st_lds);                                     // [2][THREADS]
    double* red = reinterpret_cast<double*>(pixs + 2 * lt::THREADS);                            // [8]
    float* colred = reinterpret_cast<float*>(red + 8);                                          // [4][MAX_C]
    float* zimg = colred + 4 * lt::MAX_C;                                                       // [THREADS][S]: every offset a multiple of 16 bytes
    float* timg = zimg + lt::THREADS * S;                                                       // [THREADS][S]

    const long long tiles = (a.nslot + lt::THREADS - 1) / lt::THREADS;
    double acc = 0.0;
    float colrun = 0.f;                                                                         // wave 0, lane c: column c over the block's tiles
    lt::Pieces<NV, true> in;
    float4 tv[TPRE ? NV : 1];
    StOwn own = {-1, 255u};
    int buf = 0;
    if ((long long)blockIdx.x < tiles) {
        own = st_own(a, blockIdx.x, t, pixs);
        if (CT > 0) {
            if (TPRE) { __syncthreads(); st_load_targets<NV>(a, blockIdx.x, t, pixs, tv); }
            lt::load_pieces<NV, true>(a, blockIdx.x, t, in);
        }
    }
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long g0 = tile * lt::THREADS;
        const int npx = lt::tile_rows(a.nslot, tile);
        const long long* pcur = pixs + buf * lt::THREADS;
        long long* pnext = pixs + (buf ^ 1) * lt::THREADS;
        const StOwn cur = own;
        float4 dcur[NV > 0 ? NV : 1];

        // ---- the images of this tile
        if (CT > 0) {
            lt::scatter<CT>(zimg, t, in.zv);
            if (TPRE) lt::scatter<CT>(timg, t, tv);
#pragma unroll
            for (int k = 0; k < NV; ++k) dcur[k] = in.dv[k];
            if (!TPRE) { __syncthreads(); st_fill_targets(timg, a, pcur, npx, t); }            // (pcur is visible behind the barrier)
        } else {
            lt::fill_rows(zimg, a.z + g0 * C, npx, C, S, a.zvec, t);
            __syncthreads();
            st_fill_targets(timg, a, pcur, npx, t);
        }
        // ---- the next tile's map, then its loads: in flight while this tile is worked on
        const long long next = tile + gridDim.x;
        if (next < tiles) own = st_own(a, next, t, pnext);
        __syncthreads();
        if (CT > 0 && next < tiles) {
            if (TPRE) st_load_targets<NV>(a, next, t, pnext, tv);
            lt::load_pieces<NV, true>(a, next, t, in);
        }

        // ---- the own row
        {
            float* zr = zimg + t * S;
            float* wr = timg + t * S;
            const bool part = cur.pix >= 0 && (a.all || cur.lab < (unsigned int)C);
            if (CT > 0) {
                float zreg[CD], wreg[CD];
                if (part) {
                    lt::row_in<CT>(zr, zreg);
                    lt::row_in<CT>(wr, wreg);
                    acc += (double)st_pixel<CT>(zreg, wreg, C, K, a.beta, a.coef);
                } else {
#pragma unroll
                    for (int i = 0; i < CD; ++i) wreg[i] = 0.f;
                }
                lt::row_out<CT>(wr, wreg);
            } else if (part) {
                acc += (double)st_pixel<0>(zr, wr, C, K, a.beta, a.coef);
            } else {
                for (int c = 0; c < C; ++c) wr[c] = 0.f;
            }
        }
        __syncthreads();

        // ---- drain dlogits the way it was loaded; the column sums of the contribution image
        lt::drain<CT, true>(a.d + g0 * C, npx, C, S, a.zvec, timg, t, dcur);
        lt::column_sums(timg, S, K, 0.f, colred);
        __syncthreads();                                                                        // the images are free for the next tile
        if (wave == 0) colrun = lt::fold_columns(colrun, colred);
        buf ^= 1;
    }
    lt::write_partials<false>(a, acc, 0, colrun, red);
}

// kd = (T^2 / P) sum kd_p -> term[0]; loss[0] += lambda kd; lastbias[c] += column c's sum.  Four waves, one load at a time.
__global__ __launch_bounds__(ST_RED_THREADS) void soft_targets_reduce_kernel(const double* losspart, const float* colpart, int nblocks, int K, double tt_over_p,
                                                                             float lambda, float* loss, float* term, float* lastbias)
{
    constexpr int NW = ST_RED_THREADS / 64;
    __shared__ double sh[NW];
    __shared__ float cs[NW][lt::MAX_C];
    const int t = threadIdx.x;
    double sum; unsigned long long valid; float col;
    lt::sum_partials<NW, 1, false>(losspart, nullptr, colpart, nblocks, K, 0.f, sh, nullptr, cs, sum, valid, col);
    if (t == 0) {
#pragma clang fp contract(off)
        const float kd = (float)(sum * tt_over_p);
        term[0] = kd;
        const float add = lambda * kd;
        loss[0] = loss[0] + add;
    }
    if (t < K) lastbias[t] = lastbias[t] + col;
}

}  // namespace

size_t soft_targets_scratch_bytes() { return lt::scratch_bytes(false); }

double soft_targets_bytes(long long npix, int C, int K) { return (double)npix * (4.0 * C + 4.0 * K + 1.0 + 8.0 * C); }

void launch_soft_targets(const float* logits, float* dlogits, const float* probs, const uint8_t* labels, const PixMap* map, int N, long long npix, int C,
                         int K, long long row_stride, float lambda, float temperature, int all_pixels, char* ws, float* loss, float* term,
                         float* lastbias, hipStream_t s)
{
    if (C < 1 || C > lt::MAX_C || K < 1 || K > C || row_stride < K) { defer_error(FCN8S_ERR_BAD_ARG, "soft_targets: C = %d, K = %d, row stride %lld", C, K, row_stride); return; }
    StArgs a = {};
    long long blocks = lt::plan(a, logits, dlogits, map, N, npix, C, ws, false);
    a.probs = probs; a.labels = labels; a.stride = row_stride;
    a.K = K; a.all = all_pixels;
    a.beta = 1.f / temperature;
    a.coef = lambda * (temperature / (float)npix);
    a.tvec = ((uintptr_t)probs & 15) == 0 && K % 4 == 0 && row_stride % 4 == 0;
    const size_t lds = (size_t)2 * lt::THREADS * 8 + lt::lds_bytes(a.S, 0, 2);                  // the two slot -> pixel maps in front of the frame's
    long long per_cu = (long long)(160 * 1024 / lds);                                           // blocks resident at once: 256 CUs, 160 KB of LDS each
    per_cu = per_cu > 4 ? 4 : (per_cu < 1 ? 1 : per_cu);
    if (blocks > 256 * per_cu) blocks = 256 * per_cu;
    int launched;
    if (a.zvec && C == 20 && a.tvec && K == 20) launched = lt::launch<StArgs, soft_targets_kernel<20, true>>("soft_targets", a, (int)blocks, lds, s);
    else if (a.zvec && C == 20) launched = lt::launch<StArgs, soft_targets_kernel<20, false>>("soft_targets", a, (int)blocks, lds, s);
    else launched = lt::launch<StArgs, soft_targets_kernel<0, false>>("soft_targets", a, (int)blocks, lds, s);
    if (!launched) return;
    hipLaunchKernelGGL(soft_targets_reduce_kernel, dim3(1), dim3(ST_RED_THREADS), 0, s, (const double*)a.losspart, (const float*)a.colpart, launched, K,
                       (double)temperature * (double)temperature / (double)npix, lambda, loss, term, lastbias);
}

}  // namespace fcn8s
