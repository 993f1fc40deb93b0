// Focal loss of the training objective (fcn8s_set_focal, fcn8s_op_focal_xent; the definition is in fcn8s_hip.h):
//   focal_xent_kernel         one pass over the slots of the logits: L_p = w_p (f l) per valid pixel, dlogits = the cross-entropy's gradient row times the
//                             per-pixel scalar c_p (STORED: this kernel stands where the cross-entropy's stands), per-block partial sums of the loss, of
//                             the valid pixels and of the gradient's columns
//   focal_xent_reduce_kernel  one block of 1024: the partials summed in a fixed order into the loss (or its double sum), |V| and the last bias's column sums
//
// The tile frame is loss_tile.h's.  This file adds: the label and distance code of a thread's own slot, the class weights (64 floats) and the 256-entry
// table in LDS in front of the image, the per-pixel arithmetic (expf and logf, classes summed in order, no product contracted into a sum: the header's
// definition, literally), a stored drain with pad 0.f, and the count of the valid pixels that rides with the loss.
#include "loss_tile.h"
#include <cfloat>
#include <cmath>

namespace fcn8s {
namespace {

namespace lt = loss_tile;
constexpr int FO_RED_THREADS = 1024;                   // the reduce kernel's one block

struct FoArgs : lt::Args {
    const uint8_t* labels;
    const float* cw; const uint8_t* codes; const float* ptab;   // null: all weights 1; codes and ptab both set or both null
    float gamma, gscale;                            // gscale = ce_weight / P
};

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

struct FoTerm {
    using Args = FoArgs;
    struct Own { int lab, code; };                  // the label of the own slot (-1: no valid pixel there) and its distance code
    static constexpr bool ADD = false, COUNTS = true;
    static constexpr int EXTRA = lt::MAX_C + 256;   // wsh [MAX_C], tab [256]
    static __device__ __forceinline__ float pad() { return 0.f; }
    static __device__ __forceinline__ Own none() { return {-1, 0}; }
    static __device__ __forceinline__ bool part(const Own& o) { return o.lab >= 0; }

    // lab = -1 for a slot outside the image and for an ignored pixel
    static __device__ __forceinline__ Own own(const FoArgs& a, long long tile, int t)
    {
        const long long slot = tile * lt::THREADS + t;
        const long long pix = slot < a.nslot ? slot_pixel(slot, a.pm) : -1;
        Own o = {-1, 0};
        if (pix < 0) return o;
        const int y = a.labels[pix];
        if (y >= a.C) return o;
        o.lab = y;
        if (a.codes) o.code = a.codes[pix];
        return o;
    }

    static __device__ __forceinline__ void prologue(const FoArgs& a, float* extra, int t, int C)
    {
        if (t < lt::MAX_C) extra[t] = a.cw && t < C ? a.cw[t] : 1.f;
        extra[lt::MAX_C + t] = a.ptab ? a.ptab[t] : 1.f;
    }

    template <int CT>
    static __device__ __forceinline__ void pixel(const FoArgs& a, const Own& o, float* z, int C, const float* extra, double& acc, unsigned long long& nvalid)
    {
        float w;
        {
#pragma clang fp contract(off)
            w = extra[o.lab];
            if (a.ptab) w = w * extra[lt::MAX_C + o.code];
        }
        ++nvalid;
        const float fl = fo_pixel<CT>(z, C, o.lab, w, a.gamma, a.gscale);
        acc += (double)w * (double)fl;
    }
};

template <int CT>
__global__ __launch_bounds__(lt::THREADS) void focal_xent_kernel(const FoArgs a) { lt::run_tiles<CT, FoTerm>(a); }

// With `sum_out` (the model): sum_out[0] = the double sum, which finalize_loss divides by P and rounds once; with `loss` (the op): loss[0] =
// fl(sum / P).  st (may be null): |V| into the loss state fcn8s_get_loss_stats reads.  bias (may be null): bias[c] = column c's sum.  16 waves, eight
// loads in flight (a narrower reduction measured 40 us per call).
__global__ __launch_bounds__(FO_RED_THREADS) void focal_xent_reduce_kernel(const double* __restrict__ losspart, const unsigned long long* __restrict__ validpart,
                                                                           const float* __restrict__ colpart, int nblocks, int C, double den, double* sum_out,
                                                                           float* loss, OhemState* st, float* bias)
{
    constexpr int NW = FO_RED_THREADS / 64;
    __shared__ double sh[NW];
    __shared__ unsigned long long vh[NW];
    __shared__ float cs[NW][lt::MAX_C];
    const int t = threadIdx.x;
    double sum; unsigned long long valid; float col;
    lt::sum_partials<NW, 8, true>(losspart, validpart, colpart, nblocks, C, 0.f, sh, vh, cs, sum, valid, col);
    if (t == 0) {
        if (sum_out) sum_out[0] = sum;
        if (loss) loss[0] = (float)(sum / den);
        if (st) { st->valid = valid; st->ntau = 0; st->kept = valid; st->t = 0.f; }
    }
    if (bias && t < C) bias[t] = col + 0.f;                                                     // (+0 for a batch without a valid pixel, not -0)
}

}  // namespace

size_t focal_xent_scratch_bytes() { return lt::scratch_bytes(true); }

double focal_xent_bytes(long long npix, int C, bool codes) { return (double)npix * (8.0 * C + (codes ? 2.0 : 1.0)); }

void launch_focal_xent(const float* logits, float* dlogits, const uint8_t* labels, const float* cw, const uint8_t* codes, const float* ptab, const PixMap* map,
                       int N, long long npix, int C, float gamma, float gscale, char* ws, double* sum_out, float* loss, OhemState* st, float* bias, hipStream_t s)
{
    if (C < 2 || C > lt::MAX_C || N < 1 || npix < N || !(gamma > 0.f) || !(gamma <= 8.f) || !codes != !ptab) {
        defer_error(FCN8S_ERR_BAD_ARG, "focal_xent: C = %d, N = %d, gamma = %g", C, N, (double)gamma); return;
    }
    FoArgs a = {};
    const int blocks = lt::plan(a, logits, dlogits, map, N, npix, C, ws, true);
    a.labels = labels; a.cw = cw; a.codes = codes; a.ptab = ptab;
    a.gamma = gamma; a.gscale = gscale;
    const size_t lds = lt::lds_bytes(a.S, FoTerm::EXTRA);
    const int launched = a.zvec && C == 20 ? lt::launch<FoArgs, focal_xent_kernel<20>>("focal_xent", a, blocks, lds, s)
                                           : lt::launch<FoArgs, focal_xent_kernel<0>>("focal_xent", a, blocks, lds, s);
    if (!launched) return;
    hipLaunchKernelGGL(focal_xent_reduce_kernel, dim3(1), dim3(FO_RED_THREADS), 0, s, (const double*)a.losspart, (const unsigned long long*)a.validpart,
                       (const float*)a.colpart, launched, C, (double)npix, sum_out, loss, st, bias);
}

}  // namespace fcn8s
