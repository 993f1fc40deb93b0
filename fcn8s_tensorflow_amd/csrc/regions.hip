// Connected regions of a label map (fcn8s_op_regions_label / fcn8s_op_regions_clean; the definition is in fcn8s_hip.h): the components of equal
// class under 4- or 8-connectivity, their ids (the smallest pixel index) and areas, and the cleanup that gives a small component the class of its
// largest neighbour.  Integers only; every decision is an integer min, max or add, so two runs give the same bits.
//
// Shape: a block-based union-find (Komura 2015; Playne & Hawick 2018; Allegretti et al. 2019) whose phases are split at kernel boundaries -- no
// kernel waits for another block, no ticket, no fence.  Per image, par[p] <= p always holds and a root is par[p] == p, so a root is a minimum.
//   1. rg_tile_kernel: a block of 256 threads labels one tile of RG_TH x RG_TW = 32 x 64 pixels in LDS (a wave per row, 8 rows per wave).  The labels
//      are read here, int64 as 16-byte loads of pixel pairs where the pair's address allows it.  Horizontal runs are linked by one ballot per row;
//      vertical (and diagonal) links are unions by LDS atomicMin, skipped where the pixel to the left makes the same link.  It writes par = the
//      image index of the tile-local root, the piece's pixel count at that root (0 elsewhere) and, for the cleanup, the class at that root.
//   2. rg_merge_kernel: a thread per pixel of a tile's first row / first column unites it with its equal-class neighbours in the tile above / to
//      the left by atomicMin on par.  These pixels (under 5 % of the map) are the only labels read a second time.  par is read by agent-scope
//      relaxed atomic loads: other blocks update it meanwhile.
//   3. rg_flatten_kernel: par[p] = root(p); a tile-local root that is no root adds its piece's count to its root: one integer atomic per
//      (tile, component) piece, not per pixel.
//   4. rg_area_kernel: the area of the root to every pixel.  For the cleanup the word also carries the "small" bit (bit 31) and is 0 for a
//      pixel whose label is out of range; components and small components are counted.
//   5. rg_contact_kernel (cleanup): a small pixel offers the best of its 4-neighbours that are not small to its root: atomicMax of
//      (area << 32) | (0xFFFFFFFF - id) on best[root], which holds the root's class (< 2^32) until the first offer.
//   6. rg_apply_kernel (cleanup): a small pixel whose root has an offer takes the label at the winner's id -- a pixel of a component that is not
//      small, hence not written in this round.  Relabelled components and changed pixels are counted at the roots.
//   Bounds.  A find follows strictly decreasing indices and leaves the moment an index does not decrease, whatever the memory holds; a union
//   retries only after another thread lowered a parent, the sum of its two indices falls with every retry, and it gives up after RG_MAX_RETRY
//   retries.  Either sets RG_FLAG_* in the work header (fcn8s_op_regions_status) instead of spinning.  Every index is formed from y < H, x < W.
//   Work: a header of RG_HEADER_BYTES (flags; the cleanup's counters in RG_SHARDS shards, summed per round by rg_stats_kernel), then per pixel best
//   (8 bytes), par (4) and area word (4): 16 bytes per pixel.  The labelling uses the first RG_FLAGS_BYTES alone.
#include "fcn8s_internal.h"

namespace fcn8s {

#define RG_TW 64
#define RG_TH 32
#define RG_TILE (RG_TW * RG_TH)
#define RG_THREADS 256
#define RG_ROWS_PER_WAVE (RG_TH / (RG_THREADS / 64))
#define RG_BAD 0xFFFFu                               // a label outside 0 .. 255: never equal to anything
#define RG_OUT 0xFFFEu                               // outside the image
#define RG_MAX_RETRY 4096
#define RG_FLAGS_BYTES 256                          // the part of the header that label uses: RgHeader
#define RG_SHARDS 64                                 // the cleanup's counters: RG_SHARDS x 4, a shard per 64-byte line, behind RG_SHARD_OFFSET
#define RG_SHARD_OFFSET 4096
#define RG_HEADER_BYTES 8192
#define RG_FLAG_FIND 1u                              // a parent larger than its child was met
#define RG_FLAG_UNION 2u                             // a union ran out of retries
#define RG_SMALL 0x80000000u

struct RgHeader {
    unsigned int flags;
    unsigned int pad;
    unsigned long long bad;                          // pixels whose label is outside 0 .. 255
};

#define RG_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define RG_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

template <int KIND>
__device__ __forceinline__ unsigned int rg_class(const void* __restrict__ L, long long q)
{
    if (KIND == 0) {
        const unsigned long long v = (unsigned long long)reinterpret_cast<const long long*>(L)[q];
        return v < 256ull ? (unsigned int)v : RG_BAD;
    }
    return reinterpret_cast<const uint8_t*>(L)[q];
}

// ---- LDS union-find over the RG_TILE pixels of a tile --------------------------------------------------------------------------------------
__device__ __forceinline__ int rg_lfind(const int* lp, int x)
{
    for (;;) {                                                                   // x falls with every step: at most RG_TILE steps
        const int p = __hip_atomic_load(lp + x, RG_RLX_WG);
        if (p >= x || p < 0) return x;
        x = p;
    }
}

__device__ __forceinline__ void rg_lunion(int* lp, int a, int b, unsigned int* flags)
{
    for (int it = 0; it < RG_MAX_RETRY; ++it) {
        a = rg_lfind(lp, a); b = rg_lfind(lp, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lp[a], b);
        if (old == a) return;
        a = old;                                                                 // another thread lowered lp[a] first: a + b has fallen
    }
    atomicOr(flags, RG_FLAG_UNION);
}

// ---- union-find over the pixels of one image in global memory --------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int rg_find(unsigned int* par, unsigned int x, unsigned int* flags)
{
    const unsigned int x0 = x;
    unsigned int p0 = x;
    for (;;) {                                                                   // x falls with every step
        const unsigned int p = __hip_atomic_load(par + x, RG_RLX_AGENT);
        if (x == x0) p0 = p;
        if (p >= x) {
            if (p > x) atomicOr(flags, RG_FLAG_FIND);
            break;
        }
        x = p;
    }
    if (x < p0) atomicMin(par + x0, x);                                          // a way of two steps or more: x0 straight to the root found (parents only fall)
    return x;
}

__device__ __forceinline__ void rg_union(unsigned int* par, unsigned int a, unsigned int b, unsigned int* flags)
{
    for (int it = 0; it < RG_MAX_RETRY; ++it) {
        a = rg_find(par, a, flags); b = rg_find(par, b, flags);
        if (a == b) return;
        if (a < b) { const unsigned int t = a; a = b; b = t; }
        const unsigned int old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;
    }
    atomicOr(flags, RG_FLAG_UNION);
}

// ---- 1. tile-local labelling -------------------------------------------------------------------------------------------------------------
// CLEAN: also best[local root] = class (RG_BAD for a label out of range).  areaw may be null (components only).
template <int KIND, int CONN, bool CLEAN>
__global__ __launch_bounds__(RG_THREADS) void rg_tile_kernel(const void* __restrict__ L_all, int H, int W, int tiles_x, unsigned int* __restrict__ par_all,
                                                             unsigned int* __restrict__ areaw_all, unsigned long long* __restrict__ best_all,
                                                             RgHeader* __restrict__ hdr, int count_bad)
{
    __shared__ unsigned int cls2[RG_TILE / 2];                                   // two 16-bit classes per word
    __shared__ int lp[RG_TILE];
    __shared__ int cnt[RG_TILE];
    const unsigned short* cls = reinterpret_cast<const unsigned short*>(cls2);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n = blockIdx.y, y0 = ((int)blockIdx.x / tiles_x) * RG_TH, x0 = ((int)blockIdx.x % tiles_x) * RG_TW;
    const long long P = (long long)H * W, base = (long long)n * P;

    // stage: a pixel pair per thread and step
    unsigned int nbad = 0;
#pragma unroll
    for (int j = 0; j < RG_TILE / 2 / RG_THREADS; ++j) {
        const int k = t + j * RG_THREADS, ly = k >> 5, lx = (k & 31) * 2, y = y0 + ly, x = x0 + lx;
        unsigned int c0 = RG_OUT, c1 = RG_OUT;
        if (y < H && x < W) {
            const long long q = base + (long long)y * W + x;
            if (KIND == 0) {
                const long long* ptr = reinterpret_cast<const long long*>(L_all) + q;
                if (x + 1 < W && ((uintptr_t)ptr & 15) == 0) {
                    const longlong2 v = *reinterpret_cast<const longlong2*>(ptr);
                    c0 = (unsigned long long)v.x < 256ull ? (unsigned int)v.x : RG_BAD;
                    c1 = (unsigned long long)v.y < 256ull ? (unsigned int)v.y : RG_BAD;
                } else {
                    c0 = rg_class<0>(L_all, q);
                    if (x + 1 < W) c1 = rg_class<0>(L_all, q + 1);
                }
            } else {
                c0 = rg_class<1>(L_all, q);
                if (x + 1 < W) c1 = rg_class<1>(L_all, q + 1);
            }
            nbad += (c0 == RG_BAD) + (c1 == RG_BAD);
        }
        cls2[k] = c0 | c1 << 16;
        cnt[2 * k] = 0; cnt[2 * k + 1] = 0;
    }
    if (count_bad && nbad) atomicAdd(&hdr->bad, (unsigned long long)nbad);
    __syncthreads();

    // horizontal runs: lp = the first pixel of the run, one ballot per row
#pragma unroll
    for (int r = 0; r < RG_ROWS_PER_WAVE; ++r) {
        const int ly = wv * RG_ROWS_PER_WAVE + r, i = ly * RG_TW + lane;
        const unsigned int c = cls[i];
        const bool same = lane > 0 && c < RG_OUT && cls[i - 1] == c;
        const unsigned long long starts = ~__ballot(same);                       // bit 0 is always set
        const unsigned long long below = lane == 63 ? starts : starts & ((2ull << lane) - 1ull);
        lp[i] = ly * RG_TW + (63 - __clzll((long long)below));
    }
    __syncthreads();

    // vertical and diagonal links; the pixel to the left makes the same link when it, this pixel and the two above are one class
#pragma unroll
    for (int r = 0; r < RG_ROWS_PER_WAVE; ++r) {
        const int ly = wv * RG_ROWS_PER_WAVE + r, i = ly * RG_TW + lane;
        const unsigned int c = cls[i];
        if (ly == 0 || c >= RG_OUT) continue;
        const unsigned int up = cls[i - RG_TW];
        const unsigned int lf = lane > 0 ? cls[i - 1] : RG_OUT, ul = lane > 0 ? cls[i - RG_TW - 1] : RG_OUT;
        if (up == c && !(lf == c && ul == c)) rg_lunion(lp, i, i - RG_TW, &hdr->flags);
        if (CONN == 8) {
            const unsigned int ur = lane < 63 ? cls[i - RG_TW + 1] : RG_OUT;
            if (ul == c && up != c && lf != c) rg_lunion(lp, i, i - RG_TW - 1, &hdr->flags);
            if (ur == c && up != c) rg_lunion(lp, i, i - RG_TW + 1, &hdr->flags);
        }
    }
    __syncthreads();

    // roots, and the pixel count of every piece: one LDS atomic per horizontal run
    int root[RG_ROWS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < RG_ROWS_PER_WAVE; ++r) {
        const int ly = wv * RG_ROWS_PER_WAVE + r, i = ly * RG_TW + lane;
        const unsigned int c = cls[i];
        const bool same = lane > 0 && c < RG_OUT && cls[i - 1] == c;
        const unsigned long long starts = ~__ballot(same);
        root[r] = rg_lfind(lp, i);
        if (!same && c != RG_OUT) {
            const unsigned long long above = lane == 63 ? 0ull : starts & ~((2ull << lane) - 1ull);
            const int next = above ? __ffsll((long long)above) - 1 : 64;
            atomicAdd(&cnt[root[r]], next - lane);
        }
    }
    __syncthreads();

    unsigned int* par = par_all + base;
#pragma unroll
    for (int r = 0; r < RG_ROWS_PER_WAVE; ++r) {
        const int ly = wv * RG_ROWS_PER_WAVE + r, i = ly * RG_TW + lane, y = y0 + ly, x = x0 + lane;
        if (y >= H || x >= W) continue;
        const long long p = (long long)y * W + x;
        const int rl = root[r];
        par[p] = (unsigned int)((long long)(y0 + rl / RG_TW) * W + x0 + rl % RG_TW);
        if (areaw_all) areaw_all[base + p] = rl == i ? (unsigned int)cnt[i] : 0u;
        if (CLEAN && rl == i) best_all[base + p] = cls[i];
    }
}

// ---- 2. unions across the tile borders ---------------------------------------------------------------------------------------------------
template <int KIND, int CONN>
__global__ __launch_bounds__(RG_THREADS) void rg_merge_kernel(const void* __restrict__ L_all, int H, int W, long long row_items, long long col_items,
                                                              unsigned int* __restrict__ par_all, RgHeader* __restrict__ hdr)
{
    long long idx = (long long)blockIdx.x * RG_THREADS + threadIdx.x;
    if (idx >= row_items + col_items) return;
    const long long P = (long long)H * W, base = (long long)blockIdx.y * P;
    unsigned int* par = par_all + base;
    unsigned int* flags = &hdr->flags;
    if (idx < row_items) {
        // first row of a tile: the neighbours in the row above
        const int y = ((int)(idx / W) + 1) * RG_TH, x = (int)(idx % W);
        const long long p = (long long)y * W + x;
        const unsigned int c = rg_class<KIND>(L_all, base + p);
        if (c == RG_BAD) return;
        const unsigned int up = rg_class<KIND>(L_all, base + p - W);
        const unsigned int lf = x > 0 ? rg_class<KIND>(L_all, base + p - 1) : RG_OUT;
        const unsigned int ul = x > 0 ? rg_class<KIND>(L_all, base + p - W - 1) : RG_OUT;
        if (up == c && !(x % RG_TW != 0 && lf == c && ul == c)) rg_union(par, (unsigned int)p, (unsigned int)(p - W), flags);
        if (CONN == 8) {
            const unsigned int ur = x + 1 < W ? rg_class<KIND>(L_all, base + p - W + 1) : RG_OUT;
            if (ul == c && up != c && lf != c) rg_union(par, (unsigned int)p, (unsigned int)(p - W - 1), flags);
            if (ur == c && up != c) rg_union(par, (unsigned int)p, (unsigned int)(p - W + 1), flags);
        }
    } else {
        // first column of a tile: the neighbours in the column to the left
        idx -= row_items;
        const int x = ((int)(idx / H) + 1) * RG_TW, y = (int)(idx % H);
        const long long p = (long long)y * W + x;
        const unsigned int c = rg_class<KIND>(L_all, base + p);
        if (c == RG_BAD) return;
        const unsigned int lf = rg_class<KIND>(L_all, base + p - 1);
        const unsigned int up = y > 0 ? rg_class<KIND>(L_all, base + p - W) : RG_OUT;
        const unsigned int ul = y > 0 ? rg_class<KIND>(L_all, base + p - W - 1) : RG_OUT;
        if (lf == c && !(y % RG_TH != 0 && up == c && ul == c)) rg_union(par, (unsigned int)p, (unsigned int)(p - 1), flags);
        if (CONN == 8) {
            const unsigned int dl = y + 1 < H ? rg_class<KIND>(L_all, base + p + W - 1) : RG_OUT;
            if (ul == c && up != c && lf != c) rg_union(par, (unsigned int)p, (unsigned int)(p - W - 1), flags);
            if (dl == c && lf != c) rg_union(par, (unsigned int)p, (unsigned int)(p + W - 1), flags);
        }
    }
}

// ---- 3. flatten; the pieces' counts to the roots -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void rg_flatten_kernel(long long P, unsigned int* __restrict__ par_all, unsigned int* __restrict__ areaw_all,
                                                                RgHeader* __restrict__ hdr)
{
    const long long p = (long long)blockIdx.x * RG_THREADS + threadIdx.x;
    if (p >= P) return;
    const long long base = (long long)blockIdx.y * P;
    unsigned int* par = par_all + base;
    const unsigned int r = rg_find(par, (unsigned int)p, &hdr->flags);
    __hip_atomic_store(par + p, r, RG_RLX_AGENT);                                // a shorter way to the same root for the threads that pass here
    if (areaw_all && r != (unsigned int)p) {
        const unsigned int mine = areaw_all[base + p];                           // only this thread touches the word of a pixel that is no root
        if (mine) atomicAdd(&areaw_all[base + r], mine);
    }
}

// A block's shard of the counters.  One word for all blocks was measured first: on a salted map every block of rg_area_kernel and
// rg_apply_kernel has something to add, 130 000 atomics on four addresses, and the cleanup took 1009 us where the labelling took 181.
__device__ __forceinline__ unsigned long long* rg_shard(unsigned long long* shards)
{
    return shards + ((blockIdx.x + 7u * blockIdx.y) & (RG_SHARDS - 1)) * 8;
}

// ---- 4. areas to every pixel -------------------------------------------------------------------------------------------------------------
// CLEAN: word = area | RG_SMALL, or 0 for a label out of range; stats[0] += components, stats[1] += small components.
template <bool CLEAN>
__global__ __launch_bounds__(RG_THREADS) void rg_area_kernel(long long P, const unsigned int* __restrict__ par_all, unsigned int* __restrict__ areaw_all,
                                                             const unsigned long long* __restrict__ best_all, const int* __restrict__ min_area,
                                                             unsigned long long* __restrict__ shards)
{
    __shared__ unsigned int s_cnt[2];
    if (CLEAN && threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
    if (CLEAN) __syncthreads();
    const long long p = (long long)blockIdx.x * RG_THREADS + threadIdx.x;
    if (p < P) {
        const long long base = (long long)blockIdx.y * P;
        const unsigned int r = par_all[base + p];
        // the root's own thread rewrites this word meanwhile, with the same low 31 bits
        const unsigned int a = __hip_atomic_load(areaw_all + base + r, RG_RLX_AGENT) & ~RG_SMALL;
        unsigned int w = a;
        if (CLEAN) {
            const unsigned long long c = best_all[base + r];                     // the class, written by rg_tile_kernel at every tile-local root
            if (c >= 256ull) {
                w = 0u;
            } else {
                const int m = min_area[c];
                if (m > 0 && a < (unsigned int)m) w |= RG_SMALL;
            }
            if (r == (unsigned int)p) {
                atomicAdd(&s_cnt[0], 1u);
                if (w & RG_SMALL) atomicAdd(&s_cnt[1], 1u);
            }
        }
        // a root of a label out of range has no other reader
        __hip_atomic_store(areaw_all + base + p, w, RG_RLX_AGENT);
    }
    if (CLEAN && shards) {
        __syncthreads();
        if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&rg_shard(shards)[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
    }
}

// ---- 5. offers of the neighbours that are not small ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void rg_contact_kernel(int H, int W, const unsigned int* __restrict__ par_all, const unsigned int* __restrict__ areaw_all,
                                                                unsigned long long* __restrict__ best_all)
{
    const long long P = (long long)H * W, p = (long long)blockIdx.x * RG_THREADS + threadIdx.x;
    if (p >= P) return;
    const long long base = (long long)blockIdx.y * P;
    const unsigned int* aw = areaw_all + base;
    const unsigned int w = aw[p];
    if (!(w & RG_SMALL)) return;
    const int y = (int)(p / W), x = (int)(p % W);
    const unsigned int r = par_all[base + p];
    const long long nb[4] = {y > 0 ? p - W : -1, x > 0 ? p - 1 : -1, x + 1 < W ? p + 1 : -1, y + 1 < H ? p + W : -1};
    unsigned long long key = 0ull;                                               // the best of this pixel's four first: one atomic per pixel
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (nb[k] < 0) continue;
        const unsigned int wq = aw[nb[k]];
        if ((wq & RG_SMALL) || wq == 0u) continue;                               // small (this component's own pixels among them) or out of range
        const unsigned int rq = par_all[base + nb[k]];
        const unsigned long long kq = (unsigned long long)wq << 32 | (unsigned long long)(0xFFFFFFFFu - rq);
        key = kq > key ? kq : key;
    }
    if (!key) return;
    if ((w & ~RG_SMALL) == 1u) best_all[base + r] = key;                         // a component of one pixel (most of the salt): nobody else offers
    else atomicMax(&best_all[base + r], key);
}

// ---- 6. the winners' classes ------------------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(RG_THREADS) void rg_apply_kernel(long long P, void* __restrict__ L_all, const unsigned int* __restrict__ par_all,
                                                              const unsigned int* __restrict__ areaw_all, const unsigned long long* __restrict__ best_all,
                                                              unsigned long long* __restrict__ shards)
{
    __shared__ unsigned long long s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0ull;
    __syncthreads();
    const long long p = (long long)blockIdx.x * RG_THREADS + threadIdx.x;
    if (p < P) {
        const long long base = (long long)blockIdx.y * P;
        const unsigned int w = areaw_all[base + p];
        if (w & RG_SMALL) {
            const unsigned int r = par_all[base + p];
            const unsigned long long k = best_all[base + r];
            if (k >> 32) {
                const unsigned int id = 0xFFFFFFFFu - (unsigned int)k;           // a pixel of a component that is not small: not written in this round
                if (id < (unsigned long long)P) {
                    if (KIND == 0) reinterpret_cast<long long*>(L_all)[base + p] = reinterpret_cast<const long long*>(L_all)[base + id];
                    else           reinterpret_cast<uint8_t*>(L_all)[base + p] = reinterpret_cast<const uint8_t*>(L_all)[base + id];
                    if (r == (unsigned int)p) {
                        atomicAdd(&s_cnt[0], 1ull);
                        atomicAdd(&s_cnt[1], (unsigned long long)(w & ~RG_SMALL));
                    }
                }
            }
        }
    }
    if (shards) {
        __syncthreads();
        if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&rg_shard(shards)[2 + threadIdx.x], s_cnt[threadIdx.x]);
    }
}

// the round's four counters: the sum over the shards, which are cleared for the next round
__global__ __launch_bounds__(RG_SHARDS * 4) void rg_stats_kernel(unsigned long long* __restrict__ shards, unsigned long long* __restrict__ stats)
{
    __shared__ unsigned long long sum[4];
    const int t = threadIdx.x, c = t & 3;
    if (t < 4) sum[t] = 0ull;
    __syncthreads();
    const unsigned long long v = shards[(t >> 2) * 8 + c];
    shards[(t >> 2) * 8 + c] = 0ull;
    if (v) atomicAdd(&sum[c], v);
    __syncthreads();
    if (t < 4) stats[t] = sum[t];
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
size_t regions_work_bytes(int N, int H, int W)
{
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)RG_HEADER_BYTES + (size_t)N * (size_t)H * (size_t)W * 16;
}

// the components of `labels` into par (flattened: par[p] = id), and, with areaw, the tile pieces' counts summed at the roots
template <int KIND, int CONN, bool CLEAN>
static void rg_components(const void* labels, int N, int H, int W, unsigned int* par, unsigned int* areaw, unsigned long long* best, RgHeader* hdr,
                          int count_bad, hipStream_t s)
{
    const int tiles_x = (W + RG_TW - 1) / RG_TW, tiles_y = (H + RG_TH - 1) / RG_TH;
    const long long P = (long long)H * W, row_items = (long long)(tiles_y - 1) * W, col_items = (long long)(tiles_x - 1) * H;
    const unsigned int pix_blocks = (unsigned int)((P + RG_THREADS - 1) / RG_THREADS);
    hipLaunchKernelGGL((rg_tile_kernel<KIND, CONN, CLEAN>), dim3((unsigned int)(tiles_x * tiles_y), (unsigned int)N), dim3(RG_THREADS), 0, s,
                       labels, H, W, tiles_x, par, areaw, best, hdr, count_bad);
    if (row_items + col_items > 0)
        hipLaunchKernelGGL((rg_merge_kernel<KIND, CONN>), dim3((unsigned int)((row_items + col_items + RG_THREADS - 1) / RG_THREADS), (unsigned int)N),
                           dim3(RG_THREADS), 0, s, labels, H, W, row_items, col_items, par, hdr);
    hipLaunchKernelGGL(rg_flatten_kernel, dim3(pix_blocks, (unsigned int)N), dim3(RG_THREADS), 0, s, P, par, areaw, hdr);
}

template <int KIND, int CONN>
static void rg_label(const void* labels, int N, int H, int W, int* comp, int* area, void* work, hipStream_t s)
{
    const long long P = (long long)H * W;
    const unsigned int pix_blocks = (unsigned int)((P + RG_THREADS - 1) / RG_THREADS);
    RgHeader* hdr = reinterpret_cast<RgHeader*>(work);
    rg_components<KIND, CONN, false>(labels, N, H, W, (unsigned int*)comp, (unsigned int*)area, nullptr, hdr, 1, s);
    if (area)
        hipLaunchKernelGGL((rg_area_kernel<false>), dim3(pix_blocks, (unsigned int)N), dim3(RG_THREADS), 0, s, P, (const unsigned int*)comp,
                           (unsigned int*)area, nullptr, nullptr, nullptr);
}

template <int KIND, int CONN>
static void rg_clean(void* labels, int N, int H, int W, const int* min_area, int rounds, void* work, unsigned long long* stats, hipStream_t s)
{
    const long long P = (long long)H * W;
    const unsigned int pix_blocks = (unsigned int)((P + RG_THREADS - 1) / RG_THREADS);
    RgHeader* hdr = reinterpret_cast<RgHeader*>(work);
    unsigned long long* best = reinterpret_cast<unsigned long long*>((char*)work + RG_HEADER_BYTES);
    unsigned int* par = reinterpret_cast<unsigned int*>(best + (size_t)N * P);
    unsigned int* areaw = par + (size_t)N * P;
    unsigned long long* st = stats ? reinterpret_cast<unsigned long long*>((char*)work + RG_SHARD_OFFSET) : nullptr;
    for (int r = 0; r < rounds; ++r) {
        rg_components<KIND, CONN, true>(labels, N, H, W, par, areaw, best, hdr, r == 0, s);
        hipLaunchKernelGGL((rg_area_kernel<true>), dim3(pix_blocks, (unsigned int)N), dim3(RG_THREADS), 0, s, P, par, areaw, best, min_area, st);
        hipLaunchKernelGGL(rg_contact_kernel, dim3(pix_blocks, (unsigned int)N), dim3(RG_THREADS), 0, s, H, W, par, areaw, best);
        hipLaunchKernelGGL((rg_apply_kernel<KIND>), dim3(pix_blocks, (unsigned int)N), dim3(RG_THREADS), 0, s, P, labels, par, areaw, best, st);
        if (stats) hipLaunchKernelGGL(rg_stats_kernel, dim3(1), dim3(RG_SHARDS * 4), 0, s, st, stats + 4 * r);
    }
}

static bool rg_clear(void* work, size_t bytes, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(work, 0, bytes, s);
    if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "regions: hipMemsetAsync: %s", hipGetErrorString(e)); return false; }
    return true;
}

bool regions_status(const void* work, long long* status2, hipStream_t s)
{
    RgHeader h{};
    if (hipMemcpyAsync(&h, work, sizeof h, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return false;
    status2[0] = (long long)h.flags; status2[1] = (long long)h.bad;
    return true;
}

void launch_regions_label(const void* labels, int label_kind, int N, int H, int W, int connectivity, int* comp, int* area, void* work, hipStream_t s)
{
    if (!rg_clear(work, RG_FLAGS_BYTES, s)) return;
    if (label_kind == 0) { if (connectivity == 4) rg_label<0, 4>(labels, N, H, W, comp, area, work, s); else rg_label<0, 8>(labels, N, H, W, comp, area, work, s); }
    else                 { if (connectivity == 4) rg_label<1, 4>(labels, N, H, W, comp, area, work, s); else rg_label<1, 8>(labels, N, H, W, comp, area, work, s); }
}

void launch_regions_clean(void* labels, int label_kind, int N, int H, int W, int connectivity, const int* min_area, int rounds, void* work,
                          unsigned long long* stats, hipStream_t s)
{
    if (!rg_clear(work, RG_HEADER_BYTES, s)) return;
    if (label_kind == 0) { if (connectivity == 4) rg_clean<0, 4>(labels, N, H, W, min_area, rounds, work, stats, s); else rg_clean<0, 8>(labels, N, H, W, min_area, rounds, work, stats, s); }
    else                 { if (connectivity == 4) rg_clean<1, 4>(labels, N, H, W, min_area, rounds, work, stats, s); else rg_clean<1, 8>(labels, N, H, W, min_area, rounds, work, stats, s); }
}

}  // namespace fcn8s
