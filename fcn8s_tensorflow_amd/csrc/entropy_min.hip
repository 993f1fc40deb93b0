// Entropy term of the training loss (fcn8s_set_entropy_term, fcn8s_op_entropy_term; the definition is in fcn8s_hip.h):
//   entropy_min_kernel         one pass over the slots of the logits: h_p per pixel of U, dlogits += coef (-s (b - m_p)), m_p = sum s b, per-block partial sums of
//                              h_p and of the gradient's columns
//   entropy_min_reduce_kernel  one block of 1024: the partials summed in a fixed order into the term slot, the loss and the last bias's column sums
//
// The tile frame is loss_tile.h's.  This file adds: whether a thread's own slot is a pixel of U, the per-pixel arithmetic (expf and logf, classes
// summed in order, no product contracted into a sum: the header's definition, literally), and a drain that ADDS, with pad -0.f for the columns >= K, for a
// slot outside the image and for a pixel outside U.  There is no target image: the LDS of a block is half of the soft-target kernel's.
#include "loss_tile.h"
#include <cmath>

namespace fcn8s {
namespace {

namespace lt = loss_tile;
constexpr int EM_RED_THREADS = 1024;                   // the reduce kernel's one block

struct EmArgs : lt::Args {
    const uint8_t* labels;
    long long firstpix;                             // first_image * H * W: the pixels below it belong to images < first_image
    int K, pixel_set;                               // FCN8S_ENT_*
    float coef;                                     // weight / (P log K)
};

// One pixel of U: z[0 .. n) its logits (columns >= K hold anything and are not read); on return z = coef (-s (b - sum s b)) for c < K, -0 for c >= K.
// Returns h_p.  n = CT (z is a register array, the loops unroll, the exponentials are kept) or C (z is the thread's row of the image, the
// exponentials are taken again: expf of the same float is the same float).
template <int CT>
static __device__ __forceinline__ float em_pixel(float* z, int C, int K, float coef)
{
#pragma clang fp contract(off)
    const int n = CT > 0 ? CT : C;
    float mz = -INFINITY;
#pragma unroll
    for (int c = 0; c < n; ++c) if (c < K) mz = fmaxf(mz, z[c]);
    float S = 0.f;
    float e[CT > 0 ? CT : 1];
#pragma unroll
    for (int c = 0; c < n; ++c) if (c < K) {
        const float b = z[c] - mz;                                                              // (a NaN or infinite logit: NaN from here on)
        z[c] = b;
        const float eb = expf(b);
        if (CT > 0) e[c] = eb;
        S = S + eb;
    }
    const float lS = logf(S);
    float acc = 0.f, mb = 0.f;                                                                  // sum s ls (the term), sum s b (the gradient's centre)
#pragma unroll
    for (int c = 0; c < n; ++c) if (c < K) {
        const float s = (CT > 0 ? e[c] : expf(z[c])) / S, ls = z[c] - lS;
        const float term = s * ls, sb = s * z[c];
        acc = acc + term;
        mb = mb + sb;
    }
    const float h = -acc;
#pragma unroll
    for (int c = 0; c < n; ++c) {
        if (c < K) {
            const float s = (CT > 0 ? e[c] : expf(z[c])) / S;
            const float u = z[c] - mb;                                                          // ls_c + h_p with the two logf(S) cancelled: exactly 0 on equal logits
            const float v = s * u;
            z[c] = coef * (-v);
        } else {
            z[c] = -0.f;
        }
    }
    return h;
}

struct EmTerm {
    using Args = EmArgs;
    using Own = bool;                               // the own slot is a pixel of U
    static constexpr bool ADD = true, COUNTS = false;
    static constexpr int EXTRA = 0;
    static __device__ __forceinline__ float pad() { return -0.f; }
    static __device__ __forceinline__ Own none() { return false; }
    static __device__ __forceinline__ bool part(const Own& o) { return o; }

    static __device__ __forceinline__ Own own(const EmArgs& a, long long tile, int t)
    {
        const long long slot = tile * lt::THREADS + t;
        const long long pix = slot < a.nslot ? slot_pixel(slot, a.pm) : -1;
        if (pix < a.firstpix || pix < 0) return false;
        if (a.pixel_set == FCN8S_ENT_ALL) return true;
        const unsigned int lab = a.labels[pix];
        return a.pixel_set == FCN8S_ENT_UNLABELED ? lab >= (unsigned int)a.C : lab < (unsigned int)a.C;
    }

    static __device__ __forceinline__ void prologue(const EmArgs&, float*, int, int) {}

    template <int CT>
    static __device__ __forceinline__ void pixel(const EmArgs& a, const Own&, float* z, int C, const float*, double& acc, unsigned long long&)
    {
        acc += (double)em_pixel<CT>(z, C, a.K, a.coef);
    }
};

template <int CT>
__global__ __launch_bounds__(lt::THREADS) void entropy_min_kernel(const EmArgs a) { lt::run_tiles<CT, EmTerm>(a); }

// L_ent = fl(sum h_p / (P log K)) -> term[0]; with `loss` (the model): loss[0] += fl(weight L_ent); with `bias`: bias[c] (+)= column c's sum
// (`bias_add`: the model's running bias gradient; else the op's output is set).  16 waves, eight loads in flight.  (Measured: a 256-thread block whose
// threads each walked a quarter of the blocks one load-and-add at a time cost 40 us per call, a quarter of the whole op at one 2048 x 1024 image --
// README, timing.)
__global__ __launch_bounds__(EM_RED_THREADS) void entropy_min_reduce_kernel(const double* __restrict__ losspart, const float* __restrict__ colpart, int nblocks,
                                                                            int C, double den, float weight, float* loss, float* term, float* bias, int bias_add)
{
    constexpr int NW = EM_RED_THREADS / 64;
    __shared__ double sh[NW];
    __shared__ float cs[NW][lt::MAX_C];
    const int t = threadIdx.x;
    double sum; unsigned long long valid; float col;
    lt::sum_partials<NW, 8, false>(losspart, nullptr, colpart, nblocks, C, -0.f, sh, nullptr, cs, sum, valid, col);
    if (t == 0) {
#pragma clang fp contract(off)
        const float ent = (float)(sum / den);
        term[0] = ent;
        if (loss) {
            const float add = weight * ent;
            loss[0] = loss[0] + add;
        }
    }
    if (bias && t < C) bias[t] = bias_add ? bias[t] + col : col + 0.f;                          // (the op's output: +0 for an empty U, not -0)
}

}  // namespace

size_t entropy_term_scratch_bytes() { return lt::scratch_bytes(false); }

double entropy_term_bytes(long long npix, int C) { return (double)npix * (12.0 * C + 1.0); }

float entropy_term_coef(float weight, long long npix, int K) { return (float)((double)weight / ((double)npix * std::log((double)K))); }

void launch_entropy_term(const float* logits, float* dlogits, const uint8_t* labels, const PixMap* map, int N, long long npix, int C, int K, int pixel_set,
                         int first_image, float weight, char* ws, float* loss, float* term, float* bias, int bias_add, hipStream_t s)
{
    if (C < 2 || C > lt::MAX_C || K < 2 || K > C || N < 1 || npix < N || pixel_set < 0 || pixel_set > 2 || first_image < 0) {
        defer_error(FCN8S_ERR_BAD_ARG, "entropy_term: C = %d, K = %d, N = %d, pixel set %d, first image %d", C, K, N, pixel_set, first_image); return;
    }
    EmArgs a = {};
    const int blocks = lt::plan(a, logits, dlogits, map, N, npix, C, ws, false);
    a.labels = labels;
    a.firstpix = first_image >= N ? npix : (long long)first_image * (npix / N);
    a.K = K; a.pixel_set = pixel_set;
    a.coef = entropy_term_coef(weight, npix, K);
    const size_t lds = lt::lds_bytes(a.S);
    const int launched = a.zvec && C == 20 ? lt::launch<EmArgs, entropy_min_kernel<20>>("entropy_term", a, blocks, lds, s)
                                           : lt::launch<EmArgs, entropy_min_kernel<0>>("entropy_term", a, blocks, lds, s);
    if (!launched) return;
    hipLaunchKernelGGL(entropy_min_reduce_kernel, dim3(1), dim3(EM_RED_THREADS), 0, s, (const double*)a.losspart, (const float*)a.colpart, launched, C,
                       (double)npix * std::log((double)K), weight, loss, term, bias, bias_add);
}

}  // namespace fcn8s
