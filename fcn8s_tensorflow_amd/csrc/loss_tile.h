// The tile frame of the streaming loss kernels (focal.hip, entropy_min.hip, soft_targets.hip), and slot_pixel for every kernel that walks the slots of a
// logits tensor (elementwise.hip and lovasz.hip too).  Device code: include it from .hip files only.
//
// Access shape.  A block of 256 threads takes a tile of 256 consecutive SLOTS per trip (a slot is a pixel in the plain [npix, C] layout, a place of the
// blocked layout otherwise: slot_pixel).  The tile's 256 C floats of logits and of dlogits are contiguous in slot order in both layouts and move with
// lane-contiguous loads and stores, 16 bytes per lane when the pointers allow it (use_vec; they always do inside the model: C is a multiple of 4 and
// the arena is aligned), else 4.  The logits land in an LDS image [256][S], S = C if C / 4 is odd, else C + 4 (ds_read_b128 without conflicts; S = 20
// at C = 20); on the 4-byte path S = C if C is odd, else C + 1 (row_stride).
//
// A thread owns row t of the image.  It overwrites that row by its pixel's gradient row -- by the term's pad value (0.f, or -0.f where the drain adds:
// the identity of the addition for every float) for a slot outside the image and for a pixel that takes no part -- and the block then drains the image
// to dlogits the way the logits came in (drain): every lane stores the image's 16 bytes where the logits' 16 bytes came from, or, for a term that adds
// to a gradient already there, adds them to the 16 bytes of dlogits it holds in registers (CT path) or reads back (the other paths).  dlogits is never
// staged in LDS.  The columns of the gradient image are summed by wave w over rows 64 w .. 64 w + 63, lane = column (column_sums), the four waves in
// order (fold_columns); lane c of wave 0 carries column c's running sum over the block's tiles.
//
// With C == 20 (the template parameter CT) the next tile's pieces are issued into registers (load_pieces) before the current tile is worked on.  The
// other shapes fill the image from global memory behind one more barrier (fill_rows; correct, not tuned).
//
// Grid (plan, launch): as many blocks as are resident at once (the occupancy the runtime reports for the variant, times 256 CUs), at most 1024 and at
// most one per tile, so that every block trips over the same number of tiles.
//
// Arithmetic: fp32, the per-pixel value added to a per-thread double, the block's 256 sums reduced by a shuffle tree and the four waves in order
// (write_partials), the blocks' partials by a one-block reduce kernel in a fixed order (sum_partials): no float atomics, no ticket, no fence, every
// loop bounded; two runs give the same bits, whatever the `deterministic` option says.
//
// run_tiles is the loop of a term with one image (focal, entropy); what a term adds comes in as a policy struct P:
//   Args (derived from loss_tile::Args), Own (what a thread learns about its own slot), ADD (the drain adds), COUNTS (a count rides with the double),
//   EXTRA (floats of LDS in front of the image), pad(), none(), own(a, tile, t), part(own), prologue(a, extra, t, C) and
//   pixel<CT>(a, own, z, C, extra, acc, count): z = the pixel's logits in, its gradient row out.
// The soft-target kernel has a second image and one more barrier: it keeps its own loop, built from the same pieces.
#pragma once
#include "fcn8s_internal.h"

namespace fcn8s {

// slot -> pixel index of a (possibly blocked, see PixMap) logits tensor; -1 = the slot lies outside the image
static __device__ __forceinline__ long long slot_pixel(long long slot, const PixMap& m)
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

namespace loss_tile {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 1024;
constexpr int MAX_C = 64;                               // d_lastbias holds 64 columns

__host__ __device__ constexpr int vec_stride(int C) { return (C / 4) & 1 ? C : C + 4; }
static inline int use_vec(const float* logits, const float* dlogits, int C) { return (((uintptr_t)logits | (uintptr_t)dlogits) & 15) == 0 && C % 4 == 0; }   // (null dlogits: the logits alone decide)
static inline int row_stride(int zvec, int C) { return zvec ? vec_stride(C) : (C & 1 ? C : C + 1); }

// what the frame reads of a kernel's arguments
struct Args {
    const float* z; float* d;                           // d may be null where the term's entry allows it: the loss and the column sums only
    PixMap pm;
    long long nslot;
    int C, S;                                           // S: row stride of the LDS image in floats
    int zvec;                                           // 16-byte path of logits / dlogits
    double* losspart; float* colpart; unsigned long long* validpart;    // [blocks], [blocks][MAX_C], [blocks] (a term that counts)
};

// dynamic LDS of a block: red [8] (4 doubles, then 4 counts) | colred [4][MAX_C] | `extra` floats of the term's own | `images` of [THREADS][S]
static inline size_t lds_bytes(int S, int extra = 0, int images = 1) { return 8 * 8 + (size_t)4 * MAX_C * 4 + (size_t)extra * 4 + (size_t)images * THREADS * S * 4; }
// the partials in the workspace: losspart [MAX_BLOCKS] | validpart [MAX_BLOCKS] (a term that counts) | colpart [MAX_BLOCKS][MAX_C]
static inline size_t scratch_bytes(bool counts) { return (size_t)MAX_BLOCKS * ((counts ? 16 : 8) + MAX_C * 4); }

static __device__ __forceinline__ int tile_rows(long long nslot, long long tile)
{
    const long long left = nslot - tile * THREADS;
    return left < THREADS ? (int)left : THREADS;
}

// what a thread holds of a tile before it is worked on (CT path): its pieces of the logits and, where the drain adds, of dlogits
template <int NV, bool HOLD>
struct Pieces { float4 zv[NV > 0 ? NV : 1], dv[HOLD && NV > 0 ? NV : 1]; };

template <int NV, bool HOLD>
static __device__ __forceinline__ void load_pieces(const Args& a, long long tile, int t, Pieces<NV, HOLD>& in)
{
    const long long g0 = tile * THREADS;
    const int nvec = tile_rows(a.nslot, tile) * NV;
    const float4* zs = reinterpret_cast<const float4*>(a.z + g0 * (NV * 4));
    const float4* ds = reinterpret_cast<const float4*>(a.d + g0 * (NV * 4));       // (never dereferenced without dlogits)
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = t + k * THREADS;
        const bool in_tile = i < nvec;
        in.zv[k] = in_tile ? zs[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (HOLD) in.dv[k] = in_tile && a.d ? ds[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// (CT path) the held pieces into the image [THREADS][vec_stride(CT)] (the stride a constant here: at S == CT the compiler sees that a piece lands at its own offset)
template <int CT>
static __device__ __forceinline__ void scatter(float* img, int t, const float4* v)
{
    constexpr int CD = CT > 0 ? CT : 1, S = vec_stride(CD);
#pragma unroll
    for (int k = 0; k < CT / 4; ++k) {
        const int f = (t + k * THREADS) * 4, px = f / CD, c = f - px * CD;                      // px < 256 for every k < CT / 4
        *reinterpret_cast<float4*>(img + px * S + c) = v[k];
    }
}

// the tile's npx rows of C floats at src into the image [THREADS][S]
static __device__ __forceinline__ void fill_rows(float* img, const float* src, int npx, int C, int S, int vec, int t)
{
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const int nvec = npx * (C / 4);
        for (int i = t; i < nvec; i += THREADS) {
            const int f = i * 4, px = f / C, c = f - px * C;
            *reinterpret_cast<float4*>(img + px * S + c) = s4[i];
        }
    } else {
        const int nfl = npx * C;
        for (int i = t; i < nfl; i += THREADS) {
            const int px = i / C, c = i - px * C;
            img[px * S + c] = src[i];
        }
    }
}

// (CT path) a thread's row of an image into registers and back
template <int CT>
static __device__ __forceinline__ void row_in(const float* row, float* reg)
{
#pragma unroll
    for (int i = 0; i < CT / 4; ++i) {
        const float4 q = reinterpret_cast<const float4*>(row)[i];
        reg[4 * i] = q.x; reg[4 * i + 1] = q.y; reg[4 * i + 2] = q.z; reg[4 * i + 3] = q.w;
    }
}
template <int CT>
static __device__ __forceinline__ void row_out(float* row, const float* reg)
{
#pragma unroll
    for (int i = 0; i < CT / 4; ++i)
        reinterpret_cast<float4*>(row)[i] = make_float4(reg[4 * i], reg[4 * i + 1], reg[4 * i + 2], reg[4 * i + 3]);
}

// the image to the tile's npx rows of dlogits at d, the way the logits were loaded; ADD: added to what is there (CT path: to the held pieces dcur)
template <int CT, bool ADD>
static __device__ __forceinline__ void drain(float* d, int npx, int C, int S, int vec, const float* img, int t, const float4* dcur)
{
    if (CT > 0) {
        constexpr int NV = CT / 4, CD = CT > 0 ? CT : 1, SC = vec_stride(CD);                   // (the stride a constant, as in scatter)
        float4* dst = reinterpret_cast<float4*>(d);
        const int nvec = npx * NV;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = t + k * THREADS;
            const int f = i * 4, px = f / CD, c = f - px * CD;
            const float4 g = *reinterpret_cast<const float4*>(img + px * SC + c);
            if (i < nvec) dst[i] = ADD ? make_float4(dcur[k].x + g.x, dcur[k].y + g.y, dcur[k].z + g.z, dcur[k].w + g.w) : g;
        }
    } else if (vec) {
        float4* dst = reinterpret_cast<float4*>(d);
        const int nvec = npx * (C / 4);
        for (int i = t; i < nvec; i += THREADS) {
            const int f = i * 4, px = f / C, c = f - px * C;
            const float4 g = *reinterpret_cast<const float4*>(img + px * S + c);
            if (ADD) {
                const float4 o = dst[i];
                dst[i] = make_float4(o.x + g.x, o.y + g.y, o.z + g.z, o.w + g.w);
            } else {
                dst[i] = g;
            }
        }
    } else {
        const int nfl = npx * C;
        for (int i = t; i < nfl; i += THREADS) {
            const int px = i / C, c = i - px * C;
            d[i] = ADD ? d[i] + img[px * S + c] : img[px * S + c];
        }
    }
}

// wave w sums the image's columns < ncol over rows 64 w .. 64 w + 63, from `pad`; then (behind a barrier) wave 0 folds the four waves into colrun.
// (lane and wave are taken from threadIdx here, not passed in: colred[64 wave + lane] is colred[t] only where the compiler sees both; as arguments they
// cost entropy_min_kernel<20> a register and with it a resident block per CU)
static __device__ __forceinline__ void column_sums(const float* img, int S, int ncol, float pad, float* colred)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float v = pad;
    if (lane < ncol) {
        const float* col = img + (wave * 64) * S + lane;
        for (int r = 0; r < 64; ++r) v = v + col[r * S];
    }
    colred[wave * MAX_C + lane] = v;
}
static __device__ __forceinline__ float fold_columns(float colrun, const float* colred)
{
    const int lane = threadIdx.x & 63;
    return colrun + (((colred[lane] + colred[MAX_C + lane]) + colred[2 * MAX_C + lane]) + colred[3 * MAX_C + lane]);
}

// the block's partials: the 256 doubles (and counts) by a shuffle tree and the four waves in order, wave 0's running column sums
template <bool COUNTS>
static __device__ __forceinline__ void write_partials(const Args& a, double acc, unsigned long long count, float colrun, double* red)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long* vred = reinterpret_cast<unsigned long long*>(red + 4);
    for (int o = 32; o > 0; o >>= 1) { acc += __shfl_down(acc, o, 64); if (COUNTS) count += __shfl_down(count, o, 64); }
    if (lane == 0) { red[wave] = acc; if (COUNTS) vred[wave] = count; }
    __syncthreads();
    if (t == 0) {
        a.losspart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
        if (COUNTS) a.validpart[blockIdx.x] = ((vred[0] + vred[1]) + vred[2]) + vred[3];
    }
    if (wave == 0) a.colpart[(size_t)blockIdx.x * MAX_C + lane] = colrun;
}

// the loop of a term with one image; grid: blocks (<= tiles), block: THREADS.  CT: C as a compile-time constant (next-tile loads in registers; needs
// the 16-byte path), 0 = a.C
template <int CT, class P>
static __device__ __forceinline__ void run_tiles(const typename P::Args& a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tile_lds[];
    constexpr int NV = CT / 4, CD = CT > 0 ? CT : 1;
    const int t = threadIdx.x, wave = t >> 6;
    const int C = CT > 0 ? CT : a.C, S = CT > 0 ? vec_stride(CT) : a.S;
    double* red = reinterpret_cast<double*>(tile_lds);                                          // [8]
    float* colred = reinterpret_cast<float*>(red + 8);                                          // [4][MAX_C]
    float* extra = colred + 4 * MAX_C;                                                          // [P::EXTRA]
    float* img = extra + P::EXTRA;                                                              // [THREADS][S]: the offset is a multiple of 16 bytes
    static_assert(P::EXTRA % 4 == 0, "the image starts at a multiple of 16 bytes");

    P::prologue(a, extra, t, C);                    // (the first tile's barrier below stands between these stores and their first read)

    const long long tiles = (a.nslot + THREADS - 1) / THREADS;
    double acc = 0.0;
    unsigned long long count = 0;
    float colrun = 0.f;                                                                         // wave 0, lane c: column c over the block's tiles
    Pieces<NV, P::ADD> in;
    typename P::Own own = P::none();
    if ((long long)blockIdx.x < tiles) {
        own = P::own(a, blockIdx.x, t);
        if (CT > 0) load_pieces<NV, P::ADD>(a, blockIdx.x, t, in);
    }
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long g0 = tile * THREADS;
        const int npx = tile_rows(a.nslot, tile);
        const typename P::Own cur = own;
        float4 dcur[P::ADD && NV > 0 ? NV : 1];

        // ---- the image of this tile
        if (CT > 0) {
            scatter<CT>(img, t, in.zv);
            if (P::ADD) {
#pragma unroll
                for (int k = 0; k < NV; ++k) dcur[k] = in.dv[k];
            }
        } else {
            fill_rows(img, a.z + g0 * C, npx, C, S, a.zvec, t);
        }
        // ---- the next tile's loads: in flight while this tile is worked on
        const long long next = tile + gridDim.x;
        if (next < tiles) {
            own = P::own(a, next, t);
            if (CT > 0) load_pieces<NV, P::ADD>(a, next, t, in);
        }
        __syncthreads();

        // ---- the own row
        {
            float* zr = img + t * S;
            const bool part = P::part(cur);
            if (CT > 0) {
                float zreg[CD];
                if (part) {
                    row_in<CT>(zr, zreg);
                    P::template pixel<CT>(a, cur, zreg, C, extra, acc, count);
                } else {
#pragma unroll
                    for (int i = 0; i < CD; ++i) zreg[i] = P::pad();
                }
                row_out<CT>(zr, zreg);
            } else if (part) {
                P::template pixel<0>(a, cur, zr, C, extra, acc, count);
            } else {
                for (int c = 0; c < C; ++c) zr[c] = P::pad();
            }
        }
        __syncthreads();

        // ---- drain the image to dlogits the way the logits were loaded; the column sums of the gradient image
        if (a.d) drain<CT, P::ADD>(a.d + g0 * C, npx, C, S, a.zvec, img, t, dcur);
        column_sums(img, S, C, P::pad(), colred);
        __syncthreads();                                                                        // the image is free for the next tile
        if (wave == 0) colrun = fold_columns(colrun, colred);
    }
    write_partials<P::COUNTS>(a, acc, count, colrun, red);
}

// A reduce kernel's one block of NW waves: the blocks' partials in a fixed order.  The doubles (and counts): thread t over the blocks t, t + 64 NW, ...,
// a shuffle tree, the NW waves in order -> sum, valid (in thread 0).  The columns: wave w sums column `lane` over the blocks w, w + NW, ... in order
// from `pad`, DEPTH loads in flight at a time, then the NW waves in order -> col (in the threads t < ncol).  sh [NW], vh [NW] (COUNTS), cs [NW][MAX_C]:
// the kernel's own static LDS.
template <int NW, int DEPTH, bool COUNTS>
static __device__ __forceinline__ void sum_partials(const double* losspart, const unsigned long long* validpart, const float* colpart, int nblocks, int ncol,
                                                    float pad, double* sh, unsigned long long* vh, float (*cs)[MAX_C], double& sum,
                                                    unsigned long long& valid, float& col)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double v = 0.0;
    unsigned long long nv = 0;
    for (int b = t; b < nblocks; b += NW * 64) { v += losspart[b]; if (COUNTS) nv += validpart[b]; }
    for (int o = 32; o > 0; o >>= 1) { v += __shfl_down(v, o, 64); if (COUNTS) nv += __shfl_down(nv, o, 64); }
    if (lane == 0) { sh[wave] = v; if (COUNTS) vh[wave] = nv; }
    float c = pad;
    if (lane < ncol) {
        int b = wave;
        if (DEPTH > 1) {
            for (; b + (DEPTH - 1) * NW < nblocks; b += DEPTH * NW) {
                float x[DEPTH];
#pragma unroll
                for (int j = 0; j < DEPTH; ++j) x[j] = colpart[(size_t)(b + j * NW) * MAX_C + lane];
#pragma unroll
                for (int j = 0; j < DEPTH; ++j) c = c + x[j];
            }
        }
        for (; b < nblocks; b += NW) c = c + colpart[(size_t)b * MAX_C + lane];
    }
    cs[wave][lane] = c;
    __syncthreads();
    sum = 0.0; valid = 0; col = 0.f;
    if (t == 0) {
        sum = sh[0];
        if (COUNTS) valid = vh[0];
        for (int w = 1; w < NW; ++w) { sum += sh[w]; if (COUNTS) valid += vh[w]; }
    }
    if (t < ncol) {
        col = cs[0][t];
        for (int w = 1; w < NW; ++w) col = col + cs[w][t];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------

// the frame's part of a kernel's arguments; -> one block per tile, at most MAX_BLOCKS (launch clamps to the resident ones)
static inline int plan(Args& a, const float* logits, float* dlogits, const PixMap* map, int N, long long npix, int C, char* ws, bool counts)
{
    a.z = logits; a.d = dlogits;
    a.pm = map ? *map : PixMap{0, 0, 0, 0, 0, 0};
    a.nslot = pixmap_slots(a.pm, npix, N);
    a.C = C;
    a.zvec = use_vec(logits, dlogits, C);
    a.S = row_stride(a.zvec, C);
    a.losspart = reinterpret_cast<double*>(ws);
    a.validpart = counts ? reinterpret_cast<unsigned long long*>(ws + (size_t)MAX_BLOCKS * 8) : nullptr;
    a.colpart = reinterpret_cast<float*>(ws + (size_t)MAX_BLOCKS * (counts ? 16 : 8));
    const long long tiles = (a.nslot + THREADS - 1) / THREADS;
    const long long blocks = tiles < MAX_BLOCKS ? tiles : MAX_BLOCKS;
    return blocks < 1 ? 1 : (int)blocks;
}

// launches KERNEL on no more blocks than are resident at once, so that every block trips over the same number of tiles (256 CUs; what the runtime
// reports for this instantiation and this much LDS decides) -> the blocks launched (0: refused)
template <class A, void (*KERNEL)(const A)>
static int launch(const char* who, const A& a, int blocks, size_t lds, hipStream_t s)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "%s: %zu bytes of LDS refused (%s)", who, lds, hipGetErrorString(e)); return 0; }
    }
    static int resident = 0; static size_t resident_lds = 0;
    if (!resident || resident_lds != lds) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(KERNEL), THREADS, lds) != hipSuccess || n < 1) { n = 1; (void)hipGetLastError(); }
        resident = n; resident_lds = lds;
    }
    if (blocks > 256 * resident) blocks = 256 * resident;
    hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(THREADS), lds, s, a);
    return blocks;
}

}  // namespace loss_tile
}  // namespace fcn8s
