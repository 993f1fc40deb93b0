// Entropy term of the training loss (fcn8s_set_entropy_term, fcn8s_op_entropy_term; the definition is in fcn8s_hip.h):
//   entropy_min_kernel         one pass over the slots of the logits: h_p per pixel of U, dlogits += coef (-s (b - m_p)), m_p = sum s b, per-block partial sums of
//                              h_p and of the gradient's columns
//   entropy_min_reduce_kernel  one block of 1024: the partials summed in a fixed order into the term slot, the loss and the last bias's column sums
//
// Access shape: the tile scheme of soft_targets.hip, restated here so that soft_targets.hip, temperature.hip and their objects stay byte for byte
// what they were.  A block of 256 threads takes a tile of 256 consecutive SLOTS per trip (a slot is a pixel in the plain [npix, C] layout, a place
// of the blocked layout otherwise; lov_slot_pixel's rule is restated as em_slot_pixel).  The tile's 256 C floats of logits and of dlogits are
// contiguous in slot order in both layouts and move with lane-contiguous loads and stores, 16 bytes per lane when the pointers allow it (they always
// do inside the model: C is a multiple of 4 and the arena is aligned), else 4.  The logits land in ONE LDS image [256][S], S = C if C / 4 is odd,
// else C + 4 (ds_read_b128 without conflicts; S = 20 at C = 20); on the 4-byte path S = C if C is odd, else C + 1.  There is no target image: the
// LDS of a block is half of the soft-target kernel's.
//
// A thread owns row t of the image.  It overwrites its row by the gradient contribution coef (-s_c (b_c - m_p)) -- by -0.0f, the identity of the
// addition for every float, for the columns >= K, for a slot outside the image and for a pixel outside U -- and the block then drains dlogits the
// way it was loaded: every lane adds the image's 16 bytes to the 16 bytes of dlogits it holds and stores them where they came from.  dlogits is
// never staged in LDS; without dlogits (the op's term-only call) nothing is loaded or stored.  The columns of the contribution image are summed by
// wave w over rows 64 w .. 64 w + 63, lane = column, the four waves in order; lane c of wave 0 carries column c's running sum over the block's tiles.
//
// With C == 20 (the template parameter CT) the next tile's logits and dlogits are issued into registers before the current tile is worked on.  The
// other shapes fill the image from global memory behind one more barrier (correct, not tuned).
//
// Grid: as many blocks as are resident at once (the occupancy the runtime reports for the variant, times 256 CUs), at most 1024 and at most one per
// tile, so that every block trips over the same number of tiles.
//
// Arithmetic: fp32, expf and logf, classes summed in order, no product contracted into a sum (the header's definition, literally).  h_p is added to a
// per-thread double, the block's 256 sums are reduced by a shuffle tree and the four waves in order, the blocks' partials by the reduce kernel in a
// fixed order: no float atomics, no ticket, no fence, every loop bounded; two runs give the same bits.
#include "fcn8s_internal.h"
#include <cmath>

namespace fcn8s {
namespace {

constexpr int EM_THREADS = 256;
constexpr int EM_MAX_BLOCKS = 1024;
constexpr int EM_RED_THREADS = 1024;                   // the reduce kernel's one block
constexpr int EM_MAX_C = 64;                         // d_lastbias holds 64 columns

__host__ __device__ constexpr int em_vec_stride(int C) { return (C / 4) & 1 ? C : C + 4; }

// slot -> pixel of a (possibly blocked) logits tensor, as lovasz.hip's lov_slot_pixel; -1: the slot lies outside the image
static __device__ __forceinline__ long long em_slot_pixel(long long slot, const PixMap& m)
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

struct EmArgs {
    const float* z; float* d; const uint8_t* labels;   // d may be null: the term and the column sums only
    PixMap pm;
    long long nslot, npix, firstpix;                // firstpix = first_image * H * W: the pixels below it belong to images < first_image
    int C, K, S;                                    // S: row stride of the LDS image in floats
    int zvec, pixel_set;                            // 16-byte path of logits / dlogits; FCN8S_ENT_*
    float coef;                                     // weight / (P log K)
    double* losspart; float* colpart;               // [blocks], [blocks][EM_MAX_C]
};

// what a thread holds of a tile before it is worked on
template <int NV>
struct EmIn {
    float4 zv[NV > 0 ? NV : 1], dv[NV > 0 ? NV : 1];
    bool part;                                      // slot g0 + t is a pixel of U
};

// whether the own slot of tile `tile` is a pixel of U
static __device__ __forceinline__ bool em_own(const EmArgs& a, long long tile, int t)
{
    const long long slot = tile * EM_THREADS + t;
    const long long pix = slot < a.nslot ? em_slot_pixel(slot, a.pm) : -1;
    if (pix < a.firstpix || pix < 0) return false;
    if (a.pixel_set == FCN8S_ENT_ALL) return true;
    const unsigned int lab = a.labels[pix];
    return a.pixel_set == FCN8S_ENT_UNLABELED ? lab >= (unsigned int)a.C : lab < (unsigned int)a.C;
}

// (CT path) the tile's pieces of logits and dlogits into registers
template <int NV>
static __device__ __forceinline__ void em_load(const EmArgs& a, long long tile, int t, EmIn<NV>& in)
{
    const long long g0 = tile * EM_THREADS;
    const long long left = a.nslot - g0;
    const int npx = left < EM_THREADS ? (int)left : EM_THREADS;
    const int nvec = npx * NV;
    const float4* zs = reinterpret_cast<const float4*>(a.z + g0 * (NV * 4));
    const float4* ds = reinterpret_cast<const float4*>(a.d + g0 * (NV * 4));       // (never dereferenced without dlogits)
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = t + k * EM_THREADS;
        const bool in_tile = i < nvec;
        in.zv[k] = in_tile ? zs[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        in.dv[k] = in_tile && a.d ? ds[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// the tile's npx rows of C floats at src into the image [EM_THREADS][S]
static __device__ __forceinline__ void em_fill_rows(float* img, const float* src, int npx, int C, int S, int vec, int t)
{
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const int nvec = npx * (C / 4);
        for (int i = t; i < nvec; i += EM_THREADS) {
            const int f = i * 4, px = f / C, c = f - px * C;
            *reinterpret_cast<float4*>(img + px * S + c) = s4[i];
        }
    } else {
        const int nfl = npx * C;
        for (int i = t; i < nfl; i += EM_THREADS) {
            const int px = i / C, c = i - px * C;
            img[px * S + c] = src[i];
        }
    }
}

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

// grid: blocks (<= tiles), block: EM_THREADS.  CT: C as a compile-time constant (next-tile loads in registers; needs the 16-byte path), 0 = a.C
template <int CT>
__global__ __launch_bounds__(EM_THREADS) void entropy_min_kernel(const EmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long em_lds[];
    constexpr int NV = CT / 4, CD = CT > 0 ? CT : 1;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int C = CT > 0 ? CT : a.C, S = CT > 0 ? em_vec_stride(CT) : a.S, K = a.K;
    double* red = reinterpret_cast<double*>(em_lds);                                            // [8]
    float* colred = reinterpret_cast<float*>(red + 8);                                          // [4][EM_MAX_C]
    float* img = colred + 4 * EM_MAX_C;                                                         // [EM_THREADS][S]: the offset is a multiple of 16 bytes

    const long long tiles = (a.nslot + EM_THREADS - 1) / EM_THREADS;
    double acc = 0.0;
    float colrun = 0.f;                                                                         // wave 0, lane c: column c over the block's tiles
    EmIn<NV> in;
    in.part = false;
    if ((long long)blockIdx.x < tiles) {
        in.part = em_own(a, blockIdx.x, t);
        if (CT > 0) em_load<NV>(a, blockIdx.x, t, in);
    }
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long g0 = tile * EM_THREADS;
        const long long left = a.nslot - g0;
        const int npx = left < EM_THREADS ? (int)left : EM_THREADS;
        const bool part = in.part;
        float4 dcur[NV > 0 ? NV : 1];

        // ---- the image of this tile
        if (CT > 0) {
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int f = (t + k * EM_THREADS) * 4, px = f / CD, c = f - px * CD;           // px < 256 for every k < NV
                *reinterpret_cast<float4*>(img + px * S + c) = in.zv[k];
                dcur[k] = in.dv[k];
            }
        } else {
            em_fill_rows(img, a.z + g0 * C, npx, C, S, a.zvec, t);
        }
        // ---- the next tile's loads: in flight while this tile is worked on
        const long long next = tile + gridDim.x;
        if (next < tiles) {
            in.part = em_own(a, next, t);
            if (CT > 0) em_load<NV>(a, next, t, in);
        }
        __syncthreads();

        // ---- the own row
        {
            float* zr = img + t * S;
            if (CT > 0) {
                float zreg[CT > 0 ? CT : 1];
                if (part) {
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        const float4 zq = reinterpret_cast<const float4*>(zr)[i];
                        zreg[4 * i] = zq.x; zreg[4 * i + 1] = zq.y; zreg[4 * i + 2] = zq.z; zreg[4 * i + 3] = zq.w;
                    }
                    acc += (double)em_pixel<CT>(zreg, C, K, a.coef);
                } else {
#pragma unroll
                    for (int i = 0; i < (CT > 0 ? CT : 1); ++i) zreg[i] = -0.f;
                }
#pragma unroll
                for (int i = 0; i < NV; ++i)
                    reinterpret_cast<float4*>(zr)[i] = make_float4(zreg[4 * i], zreg[4 * i + 1], zreg[4 * i + 2], zreg[4 * i + 3]);
            } else if (part) {
                acc += (double)em_pixel<0>(zr, C, K, a.coef);
            } else {
                for (int c = 0; c < C; ++c) zr[c] = -0.f;
            }
        }
        __syncthreads();

        // ---- drain dlogits the way it was loaded; the column sums of the contribution image
        if (a.d) {
            if (CT > 0) {
                float4* dst = reinterpret_cast<float4*>(a.d + g0 * C);
                const int nvec = npx * NV;
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int i = t + k * EM_THREADS;
                    const int f = i * 4, px = f / CD, c = f - px * CD;
                    const float4 g = *reinterpret_cast<const float4*>(img + px * S + c);
                    if (i < nvec) dst[i] = make_float4(dcur[k].x + g.x, dcur[k].y + g.y, dcur[k].z + g.z, dcur[k].w + g.w);
                }
            } else if (a.zvec) {
                float4* dst = reinterpret_cast<float4*>(a.d + g0 * C);
                const int nvec = npx * (C / 4);
                for (int i = t; i < nvec; i += EM_THREADS) {
                    const int f = i * 4, px = f / C, c = f - px * C;
                    const float4 g = *reinterpret_cast<const float4*>(img + px * S + c);
                    const float4 o = dst[i];
                    dst[i] = make_float4(o.x + g.x, o.y + g.y, o.z + g.z, o.w + g.w);
                }
            } else {
                float* dst = a.d + g0 * C;
                const int nfl = npx * C;
                for (int i = t; i < nfl; i += EM_THREADS) {
                    const int px = i / C, c = i - px * C;
                    dst[i] = dst[i] + img[px * S + c];
                }
            }
        }
        {
            float v = -0.f;
            if (lane < C) {
                const float* col = img + (wave * 64) * S + lane;
                for (int r = 0; r < 64; ++r) v = v + col[r * S];
            }
            colred[wave * EM_MAX_C + lane] = v;
        }
        __syncthreads();                                                                        // the image is free for the next tile
        if (wave == 0) colrun = colrun + (((colred[lane] + colred[EM_MAX_C + lane]) + colred[2 * EM_MAX_C + lane]) + colred[3 * EM_MAX_C + lane]);
    }

    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (t == 0) a.losspart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    if (wave == 0) a.colpart[(size_t)blockIdx.x * EM_MAX_C + lane] = colrun;
}

// one block of 1024: the blocks' partials in a fixed order.  L_ent = fl(sum h_p / (P log K)) -> term[0]; with `loss` (the model): loss[0] += fl(weight
// L_ent); with `bias`: bias[c] (+)= column c's sum (`bias_add`: the model's running bias gradient; else the op's output is set).  Wave w of the 16 sums
// column `lane` over the blocks w, w + 16, ... in order, eight loads in flight at a time; then the 16 waves in order.  (Measured: a 256-thread
// block whose threads each walked a quarter of the blocks one load-and-add at a time cost 40 us per call, a quarter of the whole op at one
// 2048 x 1024 image -- README, timing.)
__global__ __launch_bounds__(EM_RED_THREADS) void entropy_min_reduce_kernel(const double* __restrict__ losspart, const float* __restrict__ colpart, int nblocks,
                                                                            int C, double den, float weight, float* loss, float* term, float* bias, int bias_add)
{
    constexpr int NW = EM_RED_THREADS / 64;
    __shared__ double sh[NW];
    __shared__ float cs[NW][EM_MAX_C];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double v = 0.0;
    for (int b = t; b < nblocks; b += EM_RED_THREADS) v += losspart[b];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) sh[wave] = v;
    float c = -0.f;
    if (lane < C) {
        int b = wave;
        for (; b + 7 * NW < nblocks; b += 8 * NW) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = colpart[(size_t)(b + j * NW) * EM_MAX_C + lane];
#pragma unroll
            for (int j = 0; j < 8; ++j) c = c + x[j];
        }
        for (; b < nblocks; b += NW) c = c + colpart[(size_t)b * EM_MAX_C + lane];
    }
    cs[wave][lane] = c;
    __syncthreads();
    if (t == 0) {
#pragma clang fp contract(off)
        double sum = sh[0];
        for (int w = 1; w < NW; ++w) sum += sh[w];
        const float ent = (float)(sum / den);
        term[0] = ent;
        if (loss) {
            const float add = weight * ent;
            loss[0] = loss[0] + add;
        }
    }
    if (bias && t < C) {
        float sum = cs[0][t];
        for (int w = 1; w < NW; ++w) sum = sum + cs[w][t];
        bias[t] = bias_add ? bias[t] + sum : sum + 0.f;                                        // (the op's output: +0 for an empty U, not -0)
    }
}

size_t em_lds_bytes(int S) { return 8 * 8 + (size_t)4 * EM_MAX_C * 4 + (size_t)EM_THREADS * S * 4; }

template <int CT>
int em_launch(const EmArgs& a, int blocks, size_t lds, hipStream_t s)          // -> the blocks launched (0: refused)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&entropy_min_kernel<CT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "entropy_term: %zu bytes of LDS refused (%s)", lds, hipGetErrorString(e)); return 0; }
    }
    // no more blocks than are resident at once, so that every block trips over the same number of tiles (256 CUs; what the runtime reports decides)
    static int resident = 0; static size_t resident_lds = 0;
    if (!resident || resident_lds != lds) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(&entropy_min_kernel<CT>), EM_THREADS, lds) != hipSuccess || n < 1) { n = 1; (void)hipGetLastError(); }
        resident = n; resident_lds = lds;
    }
    if (blocks > 256 * resident) blocks = 256 * resident;
    hipLaunchKernelGGL((entropy_min_kernel<CT>), dim3(blocks), dim3(EM_THREADS), lds, s, a);
    return blocks;
}

}  // namespace

size_t entropy_term_scratch_bytes() { return (size_t)EM_MAX_BLOCKS * (8 + EM_MAX_C * 4); }

double entropy_term_bytes(long long npix, int C) { return (double)npix * (12.0 * C + 1.0); }

float entropy_term_coef(float weight, long long npix, int K) { return (float)((double)weight / ((double)npix * std::log((double)K))); }

void launch_entropy_term(const float* logits, float* dlogits, const uint8_t* labels, const PixMap* map, int N, long long npix, int C, int K, int pixel_set,
                         int first_image, float weight, char* ws, float* loss, float* term, float* bias, int bias_add, hipStream_t s)
{
    if (C < 2 || C > EM_MAX_C || K < 2 || K > C || N < 1 || npix < N || pixel_set < 0 || pixel_set > 2 || first_image < 0) {
        defer_error(FCN8S_ERR_BAD_ARG, "entropy_term: C = %d, K = %d, N = %d, pixel set %d, first image %d", C, K, N, pixel_set, first_image); return;
    }
    EmArgs a = {};
    a.z = logits; a.d = dlogits; a.labels = labels;
    a.pm = map ? *map : PixMap{0, 0, 0, 0, 0, 0};
    a.npix = npix; a.nslot = pixmap_slots(a.pm, npix, N);
    a.firstpix = first_image >= N ? npix : (long long)first_image * (npix / N);
    a.C = C; a.K = K; a.pixel_set = pixel_set;
    a.coef = entropy_term_coef(weight, npix, K);
    a.zvec = (((uintptr_t)logits | (uintptr_t)dlogits) & 15) == 0 && C % 4 == 0;                // (null dlogits: the logits alone decide)
    a.S = a.zvec ? em_vec_stride(C) : (C & 1 ? C : C + 1);
    a.losspart = reinterpret_cast<double*>(ws);
    a.colpart = reinterpret_cast<float*>(ws + (size_t)EM_MAX_BLOCKS * 8);
    const size_t lds = em_lds_bytes(a.S);
    const long long tiles = (a.nslot + EM_THREADS - 1) / EM_THREADS;
    long long blocks = tiles < EM_MAX_BLOCKS ? tiles : EM_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    const int launched = a.zvec && C == 20 ? em_launch<20>(a, (int)blocks, lds, s) : em_launch<0>(a, (int)blocks, lds, s);
    if (!launched) return;
    hipLaunchKernelGGL(entropy_min_reduce_kernel, dim3(1), dim3(EM_RED_THREADS), 0, s, (const double*)a.losspart, (const float*)a.colpart, launched, C,
                       (double)npix * std::log((double)K), weight, loss, term, bias, bias_add);
}

}  // namespace fcn8s
