// The segment pair table of panoptic quality (fcn8s_op_panoptic_pair; the definition is in fcn8s_hip.h): for every image of a batch the sparse
// joint table "pixels shared by predicted segment kp and ground-truth segment kg", from the instance map (2 B per pixel), the prediction (8 B as
// the int64 train ids `predict` returns, or 1 B as label ids) and the component ids of fcn8s_op_regions_label (4 B).  Every input byte is read
// once.  Integers only: an insert is a compare-and-swap that claims a slot for a key and an integer add on that slot's count, so the SET of
// rows (key, count) does not depend on the order in which pixels arrive; only the slot a key lands in does, hence the rows' order, which the
// callers sort away.
//
// Shape: three kernels split at kernel boundaries -- no ticket, no fence, no block waits for another, every loop is bounded.
//   1. pq_clear_kernel: the image tables' keys to PQ_EMPTY (all ones: kp = 0xFFFFFFFF would need class 31), their counts and counts[N][4] to 0.
//   2. pq_count_kernel: a lane owns PQ_PIX = 16 consecutive pixels of one image (two 16-byte loads of the instance map, eight of an int64
//      prediction, four of the components; scalar loads of an array whose address at the image's first body pixel is not 16-byte aligned, and
//      at an image's ends) and folds them into runs of equal (kp, kg) in registers, as cityscapes.hip does.  A run goes into the block's
//      private open-addressing LDS table: a 64-bit compare-and-swap on the key, then a 32-bit add on the count.  The lanes' LAST runs -- on a
//      map with long stretches, their only ones -- are first joined across the wave: neighbouring lanes with one key add once.  A run
//      that finds no LDS slot within PQ_LPROBE probes goes to the image's global table by the same insert; at block end every non-empty LDS
//      entry makes one global insert.  A constant map therefore costs one global atomic per block.  A global probe that runs out sets
//      counts[n][2] and drops the run.
//   3. pq_compact_kernel: a thread per slot; the non-empty ones draw a rank (one global atomic per block) and write rows[n][rank] when
//      rank < max_rows; counts[n][0] = rows found, counts[n][3] = the sum of all slots' counts.
//
// Sizes, and why.
//   PQ_LSLOTS = 2048 entries of 8 + 4 bytes = 24 KiB of the CU's 160 KiB: six blocks of four waves would fit a CU beside each other (the
//   registers of the int64 variant allow five), which is what a kernel that only streams and hashes needs to hide its loads; a larger table buys nothing, because a block's trips see either a few dozen
//   distinct pairs (label and instance ids are constant over long stretches) or, on noise, more pairs than any LDS table holds.
//   PQ_LPROBE = 8: a miss costs 8 LDS reads before it falls through to global memory, where the insert is correct anyway; at the load
//   factor 1/2 a linear probe of 8 fails for well under 1 % of the keys, and beyond that load the table is lost whatever the probe length.
//   PQ_GPROBE = 64 probes of the global table (16 bytes per slot: four slots per 64-byte line, so 16 lines): a table that is too small is
//   found out after 64 slots instead of a walk over all of it for every run; the caller doubles the table.  A table of at least 2 H W slots
//   is probed in full instead: an image has at most H W pairs, so that table always has an empty slot and the call cannot report an overflow.
//   Global atomics are 8 bytes wide at agent scope and execute at the L2 / memory side; what bounds them is their number, which the run
//   folding and the LDS table bring down to one per (block, pair).
//   Counts: a block's LDS count is 32 bits and an image has at most 2^26 pixels; the global count is 64 bits.
#include "fcn8s_internal.h"

namespace fcn8s {

#define PQ_THREADS 256
#define PQ_PIX 16                                    // pixels per lane per trip
#define PQ_CHUNK (PQ_THREADS * PQ_PIX)               // 4096 pixels per block per trip
#define PQ_LSLOTS 2048
#define PQ_LPROBE 8
#define PQ_GPROBE 64
#define PQ_EMPTY 0xFFFFFFFFFFFFFFFFull
#define PQ_BAD 0xFFFFFFFFu                           // kp of a pixel that is counted as bad (no kp has its low five bits all set)
#define PQ_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define PQ_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

__device__ __forceinline__ unsigned int pq_label_to_train(unsigned int L)        // labels.py id -> trainId, L < 34
{
    const unsigned long long w = L < 8 ? 0x0100000000000000ull : (L < 16 ? 0x0000050403000002ull : (L < 24 ? 0x0B0A090807000600ull
                               : (L < 32 ? 0x110000100F0E0D0Cull : 0x0000000000001312ull)));
    return (unsigned int)(w >> ((L & 7) * 8)) & 0xFFu;
}

// the predicted segment of a pixel of train id c (PQ_BAD for c >= 20) and component id comp
__device__ __forceinline__ unsigned int pq_kp(unsigned int c, unsigned int comp)
{
    if (c >= 20u) return PQ_BAD;
    return c < 12u ? c : (0x80000000u | comp << 5 | c);
}

// the ground-truth segment of an instance value v (PQ_BAD for a label beyond 33)
__device__ __forceinline__ unsigned int pq_kg(unsigned int v)
{
    const unsigned int L = v < 1000u ? v : v / 1000u;
    if (L >= 34u) return PQ_BAD;
    const unsigned int t = pq_label_to_train(L);
    if (t < 12u) return t;
    return v < 1000u ? (0x40000000u | t) : (0x80000000u | (v - L * 1000u) << 5 | t);
}

__device__ __forceinline__ unsigned int pq_hash(unsigned long long k)            // the 64-bit finaliser of MurmurHash3
{
    k ^= k >> 33; k *= 0xFF51AFD7ED558CCDull; k ^= k >> 33; k *= 0xC4CEB9FE1A85EC53ull; k ^= k >> 33;
    return (unsigned int)k;
}

__device__ __forceinline__ bool pq_lds_insert(unsigned long long* lk, unsigned int* lc, unsigned long long key, unsigned int n)
{
    unsigned int s = pq_hash(key) & (PQ_LSLOTS - 1);
#pragma unroll 1
    for (int i = 0; i < PQ_LPROBE; ++i) {
        unsigned long long k = __hip_atomic_load(lk + s, PQ_RLX_WG);
        if (k == PQ_EMPTY) { k = atomicCAS(lk + s, PQ_EMPTY, key); if (k == PQ_EMPTY) k = key; }
        if (k == key) { atomicAdd(lc + s, n); return true; }
        s = (s + 1) & (PQ_LSLOTS - 1);
    }
    return false;
}

// tab: [slots] {key, count} of one image; slots is a power of two
__device__ __forceinline__ bool pq_global_insert(unsigned long long* tab, unsigned int mask, unsigned int limit, unsigned long long key, unsigned long long n)
{
    unsigned int s = pq_hash(key) & mask;
#pragma unroll 1
    for (unsigned int i = 0; i < limit; ++i) {
        unsigned long long* slot = tab + 2 * (size_t)s;
        unsigned long long k = __hip_atomic_load(slot, PQ_RLX_AGENT);
        if (k == PQ_EMPTY) { k = atomicCAS(slot, PQ_EMPTY, key); if (k == PQ_EMPTY) k = key; }
        if (k == key) { atomicAdd(slot + 1, n); return true; }
        s = (s + 1) & mask;
    }
    return false;
}

struct PqBlock {
    unsigned long long* lk;                          // [PQ_LSLOTS] LDS keys
    unsigned int* lc;                                // [PQ_LSLOTS] LDS counts
    unsigned long long* tab;                         // the image's global table
    unsigned long long* counts;                      // the image's counts[4]
    unsigned int mask, limit;
};

__device__ __forceinline__ void pq_run(const PqBlock& b, unsigned int kp, unsigned int kg, unsigned int n, unsigned int& nbad)
{
    if (n == 0) return;
    if (kp == PQ_BAD) { nbad += n; return; }
    const unsigned long long key = (unsigned long long)kp << 32 | kg;
    if (pq_lds_insert(b.lk, b.lc, key, n)) return;
    if (!pq_global_insert(b.tab, b.mask, b.limit, key, n)) atomicOr(b.counts + 2, 1ull);
}

// The 16 (m < 16 at an image's ends) consecutive pixels at pixel q of the image: loads, keys, runs.  Every lane of the wave calls this, with
// m = 0 when it has no pixels.  wide: bit 0 / 1 / 2 = 16-byte loads of inst / pred / comp are aligned at q; only looked at when m == 16.
template <int KIND>
__device__ __forceinline__ void pq_group(const uint16_t* __restrict__ inst, const void* __restrict__ pred, const int* __restrict__ comp,
                                         long long q, int m, int wide, const PqBlock& b, unsigned int& nbad)
{
    unsigned int v[PQ_PIX], c[PQ_PIX], cp[PQ_PIX];
    const bool full = m == PQ_PIX;
    if (full && (wide & 1)) {
        const uint4 a0 = *reinterpret_cast<const uint4*>(inst + q), a1 = *reinterpret_cast<const uint4*>(inst + q + 8);
        const unsigned int vs[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int i = 0; i < PQ_PIX; ++i) v[i] = (vs[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu;
    } else {
#pragma unroll
        for (int i = 0; i < PQ_PIX; ++i) v[i] = i < m ? (unsigned int)inst[q + i] : 0u;
    }
    if (KIND == 0) {
        const long long* pl = reinterpret_cast<const long long*>(pred) + q;
        if (full && (wide & 2)) {
            const uint4* pp = reinterpret_cast<const uint4*>(pl);
            uint4 pw[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) pw[i] = pp[i];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                c[2 * i] = (pw[i].y == 0u && pw[i].x < 20u) ? pw[i].x : 255u;
                c[2 * i + 1] = (pw[i].w == 0u && pw[i].z < 20u) ? pw[i].z : 255u;
            }
        } else {
#pragma unroll
            for (int i = 0; i < PQ_PIX; ++i) {
                c[i] = 255u;
                if (i < m) { const unsigned long long a = (unsigned long long)pl[i]; c[i] = a < 20ull ? (unsigned int)a : 255u; }
            }
        }
    } else {
        const uint8_t* pb = reinterpret_cast<const uint8_t*>(pred) + q;
        unsigned int lab[PQ_PIX];
        if (full && (wide & 2)) {
            const uint4 pw = *reinterpret_cast<const uint4*>(pb);
            const unsigned int pws[4] = {pw.x, pw.y, pw.z, pw.w};
#pragma unroll
            for (int i = 0; i < PQ_PIX; ++i) lab[i] = (pws[i >> 2] >> ((i & 3) * 8)) & 0xFFu;
        } else {
#pragma unroll
            for (int i = 0; i < PQ_PIX; ++i) lab[i] = i < m ? (unsigned int)pb[i] : 255u;
        }
#pragma unroll
        for (int i = 0; i < PQ_PIX; ++i) c[i] = lab[i] < 34u ? pq_label_to_train(lab[i]) : 255u;
    }
    if (full && (wide & 4)) {
        const uint4* cw = reinterpret_cast<const uint4*>(comp + q);
#pragma unroll
        for (int i = 0; i < 4; ++i) { const uint4 w = cw[i]; cp[4 * i] = w.x; cp[4 * i + 1] = w.y; cp[4 * i + 2] = w.z; cp[4 * i + 3] = w.w; }
    } else {
#pragma unroll
        for (int i = 0; i < PQ_PIX; ++i) cp[i] = i < m ? (unsigned int)comp[q + i] : 0u;
    }

    unsigned int ckp = PQ_BAD, ckg = 0u, n = 0u;
#pragma unroll
    for (int i = 0; i < PQ_PIX; ++i) {
        if (i < m) {
            unsigned int kp = pq_kp(c[i], cp[i]);
            const unsigned int kg = pq_kg(v[i]);
            if (kg == PQ_BAD) kp = PQ_BAD;
            const unsigned int kgn = kp == PQ_BAD ? 0u : kg;                     // one key for every bad pixel
            if (n != 0u && kp == ckp && kgn == ckg) { ++n; }
            else { pq_run(b, ckp, ckg, n, nbad); ckp = kp; ckg = kgn; n = 1u; }
        }
    }
    // The lanes' last runs.  The lanes of a wave hold consecutive pixels, so equal keys sit in stretches of lanes: the first lane of a stretch
    // adds for all of it (the stretch's sum is a difference of the wave's prefix sums).
    if (n != 0u && ckp == PQ_BAD) { nbad += n; n = 0u; }
    const unsigned long long have = __ballot(n != 0u);
    if (have == 0ull) return;
    const int lane = threadIdx.x & 63;
    const unsigned int pkp = __shfl_up(ckp, 1, 64), pkg = __shfl_up(ckg, 1, 64), pn = __shfl_up(n, 1, 64);
    const bool first = n != 0u && (lane == 0 || pn == 0u || pkp != ckp || pkg != ckg);
    const unsigned long long stops = __ballot(first) | ~have;                    // lanes where a stretch begins, and lanes without a run
    unsigned int pre = n;                                                        // inclusive prefix sum over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int up = __shfl_up(pre, d, 64);
        if (lane >= d) pre += up;
    }
    const unsigned long long above = lane == 63 ? 0ull : stops & ~((2ull << lane) - 1ull);
    const int last = above ? __ffsll((long long)above) - 2 : 63;                 // the lane in front of the next stop: the end of this lane's stretch
    const unsigned int pre_last = __shfl(pre, last, 64);
    if (first) pq_run(b, ckp, ckg, pre_last - pre + n, nbad);
}

__global__ __launch_bounds__(PQ_THREADS) void pq_clear_kernel(unsigned long long* __restrict__ work, long long entries, unsigned long long* __restrict__ counts, int ncounts)
{
    const long long i = (long long)blockIdx.x * PQ_THREADS + threadIdx.x;
    if (i < entries) { ulonglong2 e; e.x = PQ_EMPTY; e.y = 0ull; reinterpret_cast<ulonglong2*>(work)[i] = e; }
    if (i < ncounts) counts[i] = 0ull;
}

// grid (blocks per image, N)
template <int KIND>
__global__ __launch_bounds__(PQ_THREADS) void pq_count_kernel(const uint16_t* __restrict__ inst_all, const void* __restrict__ pred_all, const int* __restrict__ comp_all,
                                                              long long P, unsigned long long* __restrict__ work, unsigned int slots, unsigned int limit,
                                                              unsigned long long* __restrict__ counts)
{
    __shared__ unsigned long long lk[PQ_LSLOTS];
    __shared__ unsigned int lc[PQ_LSLOTS];
    __shared__ unsigned int s_bad;
    const int t = threadIdx.x, n = blockIdx.y;
    for (int i = t; i < PQ_LSLOTS; i += PQ_THREADS) { lk[i] = PQ_EMPTY; lc[i] = 0u; }
    if (t == 0) s_bad = 0u;
    __syncthreads();

    const long long base = (long long)n * P;
    const uint16_t* inst = inst_all + base;
    const int* comp = comp_all + base;
    const void* pred = KIND == 0 ? (const void*)(reinterpret_cast<const long long*>(pred_all) + base)
                                 : (const void*)(reinterpret_cast<const uint8_t*>(pred_all) + base);
    PqBlock b;
    b.lk = lk; b.lc = lc; b.tab = work + 2 * (size_t)n * slots; b.counts = counts + 4 * (size_t)n; b.mask = slots - 1u; b.limit = limit;

    // The body starts at the image's first pixel whose index in the batch is a multiple of 16, so that buffers that are 16-byte aligned take
    // wide loads whatever P is; an array that is not aligned there takes scalar loads.
    long long head = (16 - (base & 15)) & 15;
    if (head > P) head = P;
    int wide = 0;
    if (((uintptr_t)(inst + head) & 15) == 0) wide |= 1;
    if (((uintptr_t)(KIND == 0 ? (const void*)(reinterpret_cast<const long long*>(pred) + head) : (const void*)(reinterpret_cast<const uint8_t*>(pred) + head)) & 15) == 0) wide |= 2;
    if (((uintptr_t)(comp + head) & 15) == 0) wide |= 4;
    const long long body = P - head;
    const long long nchunks = (body + PQ_CHUNK - 1) / PQ_CHUNK;
    unsigned int nbad = 0;
    for (long long ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {             // the same trips for every lane of the block
        const long long q = head + ch * PQ_CHUNK + (long long)t * PQ_PIX;
        const long long left = P - q;
        pq_group<KIND>(inst, pred, comp, q, left >= PQ_PIX ? PQ_PIX : (left > 0 ? (int)left : 0), wide, b, nbad);
    }
    if (blockIdx.x == 0 && t < 64 && head > 0)                                   // (the whole first wave: pq_group is a wave's call)
        pq_group<KIND>(inst, pred, comp, 0, t == 0 ? (int)head : 0, 0, b, nbad);
    if (nbad) atomicAdd(&s_bad, nbad);
    __syncthreads();

    for (int i = t; i < PQ_LSLOTS; i += PQ_THREADS) {
        const unsigned long long key = lk[i];
        if (key != PQ_EMPTY && !pq_global_insert(b.tab, b.mask, b.limit, key, (unsigned long long)lc[i])) atomicOr(b.counts + 2, 1ull);
    }
    if (t == 0 && s_bad) atomicAdd(b.counts + 1, (unsigned long long)s_bad);
}

// grid (slot blocks, N): a thread per slot
__global__ __launch_bounds__(PQ_THREADS) void pq_compact_kernel(const unsigned long long* __restrict__ work, unsigned int slots, long long* __restrict__ rows,
                                                                long long max_rows, unsigned long long* __restrict__ counts)
{
    __shared__ unsigned int s_rows;
    __shared__ unsigned long long s_pix, s_base;
    const int t = threadIdx.x, n = blockIdx.y, lane = t & 63;
    if (t == 0) { s_rows = 0u; s_pix = 0ull; }
    __syncthreads();
    const unsigned int s = blockIdx.x * PQ_THREADS + t;
    unsigned long long key = PQ_EMPTY, cnt = 0ull;
    if (s < slots) {
        const ulonglong2 e = reinterpret_cast<const ulonglong2*>(work)[(size_t)n * slots + s];
        key = e.x; cnt = e.y;
    }
    const bool valid = key != PQ_EMPTY;
    const unsigned long long ball = __ballot(valid);
    const unsigned int before = (unsigned int)__popcll(ball & ((1ull << lane) - 1ull));
    unsigned int wave_base = 0u;
    if (lane == 0 && ball) wave_base = atomicAdd(&s_rows, (unsigned int)__popcll(ball));
    wave_base = __shfl(wave_base, 0, 64);
    if (valid && cnt) atomicAdd(&s_pix, cnt);
    __syncthreads();
    if (t == 0) {
        s_base = s_rows ? atomicAdd(counts + 4 * (size_t)n, (unsigned long long)s_rows) : 0ull;
        if (s_pix) atomicAdd(counts + 4 * (size_t)n + 3, s_pix);
    }
    __syncthreads();
    if (valid) {
        const unsigned long long rank = s_base + wave_base + before;
        if (rank < (unsigned long long)max_rows) {
            long long* o = rows + ((size_t)n * (size_t)max_rows + rank) * 3;
            o[0] = (long long)(key >> 32); o[1] = (long long)(key & 0xFFFFFFFFull); o[2] = (long long)cnt;
        }
    }
}

size_t panoptic_work_bytes(int N, long long slots)
{
    if (N <= 0 || slots < 1 || slots > (1LL << 28) || (slots & (slots - 1))) return 0;
    return (size_t)N * (size_t)slots * 16;
}

void launch_panoptic_pair(const uint16_t* inst, const void* pred, int pred_kind, const int* comp, int N, int H, int W, void* work, long long slots,
                          long long* rows, long long max_rows, unsigned long long* counts, hipStream_t s)
{
    const long long P = (long long)H * W, entries = (long long)N * slots;
    const long long clear_items = entries > 4LL * N ? entries : 4LL * N;
    hipLaunchKernelGGL(pq_clear_kernel, dim3((unsigned int)((clear_items + PQ_THREADS - 1) / PQ_THREADS)), dim3(PQ_THREADS), 0, s,
                       (unsigned long long*)work, entries, counts, 4 * N);
    // Five blocks fit a CU beside each other: at most one such round of the 256 CUs, and every block of an image the same number of trips
    // (1536 blocks for 16 x 128 chunks gave a third of them a second trip that the others waited for: 85 us on Cityscapes-like maps and 53 us
    // on constant ones, where 16 x 64 blocks of two trips each take 73 and 45).
    const long long nchunks = (P + PQ_CHUNK - 1) / PQ_CHUNK;
    const long long target = N >= 1280 ? 1 : 1280 / N;
    const long long trips = (nchunks + target - 1) / target;
    const long long blocks = (nchunks + trips - 1) / trips;
    const unsigned int limit = (unsigned int)(slots >= 2 * P ? slots : (slots < PQ_GPROBE ? slots : PQ_GPROBE));
    if (pred_kind == 0)
        hipLaunchKernelGGL((pq_count_kernel<0>), dim3((unsigned int)blocks, (unsigned int)N), dim3(PQ_THREADS), 0, s, inst, pred, comp, P,
                           (unsigned long long*)work, (unsigned int)slots, limit, counts);
    else
        hipLaunchKernelGGL((pq_count_kernel<1>), dim3((unsigned int)blocks, (unsigned int)N), dim3(PQ_THREADS), 0, s, inst, pred, comp, P,
                           (unsigned long long*)work, (unsigned int)slots, limit, counts);
    hipLaunchKernelGGL(pq_compact_kernel, dim3((unsigned int)((slots + PQ_THREADS - 1) / PQ_THREADS), (unsigned int)N), dim3(PQ_THREADS), 0, s,
                       (const unsigned long long*)work, (unsigned int)slots, rows, max_rows, counts);
}

}  // namespace fcn8s
