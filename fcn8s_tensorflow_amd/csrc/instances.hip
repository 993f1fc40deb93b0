// The instance pair table of instance-level AP (fcn8s_op_instance_pair; the definition is in fcn8s_hip.h): for every image of a batch the sparse
// joint table "pixels shared by predicted instance kp and ground-truth value v" with, per row, the sum of the fixed-point confidence terms of
// its pixels.  Inputs per pixel: the softmax row (4 C B, of which one float is used), the label byte, the component id (4 B) and the
// instance value (2 B, or none).  Every input byte is read once.  Integers only: an insert is a compare-and-swap that claims a slot for a
// key and integer adds on that slot's count and sum, so the SET of rows does not depend on the order in which pixels arrive; only the slot a
// key lands in does, hence the rows' order, which the callers sort away.
//
// Shape: panoptic.hip's hash scheme, restated here so that that file stays what it is.  Three kernels split at kernel boundaries -- no
// ticket, no fence, no block waits for another, every loop is bounded.
//   1. in_clear_kernel: the image tables' keys to IN_EMPTY (all ones: no kp has its low five bits all set), their counts, their sums and
//      counts[N][5] to 0.
//   2. in_count_kernel: grid (blocks per image, N).  A block of 256 threads takes a tile of 256 consecutive pixels of its image per trip and
//      brings the tile's 256 C floats in the way reliability.hip does: lane-contiguous loads (16 bytes per lane when the tile's first row is
//      16-byte aligned and C % 4 == 0, 4 bytes per lane otherwise: C = 21, offset pointers), written to an LDS image [256][S] at that file's
//      conflict-free row stride; with C == 20 on the 16-byte path the next tile's loads are in flight while the current one is counted.
//      Thread t owns pixel t of the tile: it picks image[t][label] out of LDS, one ds_read_b32 (a stride that is a multiple of 4 but not of
//      8 floats is 4-way conflicted for a b32 read of a FIXED column; the column here is the pixel's label, which differs from lane to lane
//      only where the prediction changes -- on constant stretches it is the conflicted case, 4 passes of one read per tile, which is noise
//      next to the tile's 20 KiB of fill).  A row stride of more than IN_MAX_STRIDE floats does not fit the image beside the table: such C
//      read their one float per pixel from global memory.  The three maps are read with one scalar load per lane (64, 256 and 128
//      consecutive bytes per wave), so any alignment of them is allowed.
//      Runs.  The row image puts consecutive pixels on consecutive lanes, not into one lane's registers, so runs of equal (kp, v) are
//      folded across the wave instead: the first lane of a stretch of equal keys inserts for all of it -- the stretch's pixel count is a
//      lane distance and its 64-bit sum a difference of the wave's prefix sums.  A run goes into the block's private open-addressing LDS
//      table: a 64-bit compare-and-swap on the key, a 32-bit add on the count, a 64-bit add on the sum.  A run that finds no LDS slot
//      within IN_LPROBE probes goes to the image's global table by the same insert; at block end every non-empty LDS entry makes one global
//      insert.  A global probe that runs out sets counts[n][2] and drops the run.
//   3. in_compact_kernel: a thread per slot; the non-empty ones draw a rank (one global atomic per block) and write rows[n][rank] when
//      rank < max_rows; counts[n][0] = rows found, counts[n][3] = the sum of all slots' counts.
//
// Sizes.  IN_LSLOTS = 1024 entries of 8 + 4 + 8 bytes = 20 KiB; with the 20 KiB image of C = 20 four blocks fit a CU's 160 KiB.  A block's
// trips see a few dozen distinct pairs on a segmentation map, or, on noise, more than any LDS table holds.  IN_LPROBE, IN_GPROBE and the
// "a table of at least 2 H W slots is probed in full and cannot overflow" rule are panoptic.hip's.  A global slot is 32 bytes {key, count,
// sum, unused}: two aligned 16-byte stores clear it.  A block takes at least IN_MIN_TRIPS tiles where the image has them, so that the
// table's setup and flush (1024 slots each) are paid once per 2048 pixels.
// Bounds: a block's LDS count is 32 bits and an image has at most 2^26 pixels; a term is at most 2^24, so a sum stays below 2^51.
#include "fcn8s_internal.h"

namespace fcn8s {

#define IN_THREADS 256
#define IN_LSLOTS 1024
#define IN_LPROBE 8
#define IN_GPROBE 64
#define IN_MAX_STRIDE 40                             // floats per row of the LDS image: 40 KiB for the tile, 60 KiB with the table
#define IN_MIN_TRIPS 8
#define IN_EMPTY 0xFFFFFFFFFFFFFFFFull
#define IN_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define IN_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

struct InArgs {
    const float* prob; const uint8_t* labels; const int* comp; const uint16_t* inst;      // inst may be null: v = 0
    long long P;
    int C, S;                                        // S: row stride of the LDS image in floats, 0 = the float is read from global memory
    unsigned long long* work; unsigned int slots, limit;
    unsigned long long* counts;
};

// row stride of the LDS image on the 16-byte path (reliability.hip has the rule)
__host__ __device__ constexpr int in_vec_stride(int C) { return (C / 4) & 1 ? C : C + 4; }

__device__ __forceinline__ unsigned int in_hash(unsigned long long k)            // the 64-bit finaliser of MurmurHash3
{
    k ^= k >> 33; k *= 0xFF51AFD7ED558CCDull; k ^= k >> 33; k *= 0xC4CEB9FE1A85EC53ull; k ^= k >> 33;
    return (unsigned int)k;
}

__device__ __forceinline__ bool in_lds_insert(unsigned long long* lk, unsigned int* lc, unsigned long long* ls, unsigned long long key,
                                              unsigned int n, unsigned long long sum)
{
    unsigned int s = in_hash(key) & (IN_LSLOTS - 1);
#pragma unroll 1
    for (int i = 0; i < IN_LPROBE; ++i) {
        unsigned long long k = __hip_atomic_load(lk + s, IN_RLX_WG);
        if (k == IN_EMPTY) { k = atomicCAS(lk + s, IN_EMPTY, key); if (k == IN_EMPTY) k = key; }
        if (k == key) { atomicAdd(lc + s, n); if (sum) atomicAdd(ls + s, sum); return true; }
        s = (s + 1) & (IN_LSLOTS - 1);
    }
    return false;
}

// tab: [slots] {key, count, sum, unused} of one image; slots is a power of two
__device__ __forceinline__ bool in_global_insert(unsigned long long* tab, unsigned int mask, unsigned int limit, unsigned long long key,
                                                 unsigned long long n, unsigned long long sum)
{
    unsigned int s = in_hash(key) & mask;
#pragma unroll 1
    for (unsigned int i = 0; i < limit; ++i) {
        unsigned long long* slot = tab + 4 * (size_t)s;
        unsigned long long k = __hip_atomic_load(slot, IN_RLX_AGENT);
        if (k == IN_EMPTY) { k = atomicCAS(slot, IN_EMPTY, key); if (k == IN_EMPTY) k = key; }
        if (k == key) { atomicAdd(slot + 1, n); if (sum) atomicAdd(slot + 2, sum); return true; }
        s = (s + 1) & mask;
    }
    return false;
}

// what a thread holds of a tile before it is counted: its pixel's label, component and instance value, and (NV > 0) its NV 16-byte pieces of the tile's rows
template <int NV>
struct InIn {
    float4 pv[NV > 0 ? NV : 1];
    unsigned int lab, comp, v;
};

// tile: index of the tile in the image; rows: the image's softmax rows
template <int NV>
__device__ __forceinline__ void in_load(const InArgs& a, const float* __restrict__ rows, const uint8_t* __restrict__ labels, const int* __restrict__ comp,
                                        const uint16_t* __restrict__ inst, long long tile, int t, InIn<NV>& in)
{
    const long long g0 = tile * IN_THREADS;
    const long long left = a.P - g0;
    const int npx = left < IN_THREADS ? (int)left : IN_THREADS;
    if (NV > 0) {
        const float4* src = reinterpret_cast<const float4*>(rows + g0 * (NV * 4));
        const int nvec = npx * NV;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = t + k * IN_THREADS;
            in.pv[k] = i < nvec ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    in.lab = 255u; in.comp = 0u; in.v = 0u;
    if (t < npx) {
        in.lab = labels[g0 + t];
        in.comp = (unsigned int)comp[g0 + t];
        if (inst) in.v = inst[g0 + t];
    }
}

// grid (blocks per image, N), block: IN_THREADS.  VEC: the 16-byte path; CT: C as a compile-time constant (next-tile loads in registers), 0 = a.C
template <bool VEC, int CT>
__global__ __launch_bounds__(IN_THREADS) void in_count_kernel(const InArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float in_stage[];             // [IN_THREADS][S]
    __shared__ unsigned long long lk[IN_LSLOTS];
    __shared__ unsigned long long ls[IN_LSLOTS];
    __shared__ unsigned int lc[IN_LSLOTS];
    __shared__ unsigned int s_bad, s_badq;
    constexpr int NV = CT / 4;
    const int t = threadIdx.x, lane = t & 63, n = blockIdx.y;
    const int C = CT > 0 ? CT : a.C, S = CT > 0 ? in_vec_stride(CT) : a.S;
    for (int i = t; i < IN_LSLOTS; i += IN_THREADS) { lk[i] = IN_EMPTY; ls[i] = 0ull; lc[i] = 0u; }
    if (t == 0) { s_bad = 0u; s_badq = 0u; }
    __syncthreads();

    const long long base = (long long)n * a.P;
    const float* rows = a.prob + base * C;
    const uint8_t* labels = a.labels + base;
    const int* comp = a.comp + base;
    const uint16_t* inst = a.inst ? a.inst + base : nullptr;
    unsigned long long* tab = a.work + 4 * (size_t)n * a.slots;
    unsigned long long* counts = a.counts + 5 * (size_t)n;
    const unsigned int mask = a.slots - 1u, limit = a.limit;

    const long long tiles = (a.P + IN_THREADS - 1) / IN_THREADS;
    unsigned int nbad = 0u, nbadq = 0u;
    InIn<NV> in;
    if ((long long)blockIdx.x < tiles) in_load<NV>(a, rows, labels, comp, inst, blockIdx.x, t, in);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {         // the same trips for every lane of the block
        const long long g0 = tile * IN_THREADS;
        const long long left = a.P - g0;
        const int npx = left < IN_THREADS ? (int)left : IN_THREADS;
        if (S > 0) {
            if (NV > 0) {
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int f = (t + k * IN_THREADS) * 4, px = f / C, c = f - px * C;        // px < 256 for every k < NV
                    *reinterpret_cast<float4*>(in_stage + px * S + c) = in.pv[k];
                }
            } else if (VEC) {
                const float4* src = reinterpret_cast<const float4*>(rows + g0 * C);
                const int nvec = npx * (C / 4);
                for (int i = t; i < nvec; i += IN_THREADS) {
                    const int f = i * 4, px = f / C, c = f - px * C;
                    *reinterpret_cast<float4*>(in_stage + px * S + c) = src[i];
                }
            } else {
                const float* src = rows + g0 * C;
                const int nfl = npx * C, dq = IN_THREADS / C, dr = IN_THREADS % C;
                int px = t / C, c = t - px * C;
                for (int i = t; i < nfl; i += IN_THREADS) {
                    in_stage[px * S + c] = src[i];
                    px += dq; c += dr;
                    if (c >= C) { c -= C; ++px; }
                }
            }
            __syncthreads();
        }
        const unsigned int lab = in.lab, cp = in.comp, v = in.v;
        const long long next = tile + gridDim.x;
        if (next < tiles) in_load<NV>(a, rows, labels, comp, inst, next, t, in);  // in flight while this tile is counted

        const bool have = t < npx;
        const bool thing = have && lab >= 12u && lab < 20u;                      // 12 .. 19 < 20 <= C: the row holds the label's column
        unsigned long long key = IN_EMPTY, term = 0ull;
        if (have) {
            if (lab >= 20u) ++nbad;
            const unsigned int kp = thing ? (0x80000000u | cp << 5 | lab) : 0u;
            key = (unsigned long long)kp << 32 | v;
        }
        if (thing) {
            const float q = S > 0 ? in_stage[t * S + (int)lab] : rows[(g0 + t) * C + lab];
            if (q >= 0.f && q <= 1.f) term = (unsigned long long)(long long)rintf(q * 16777216.f);
            else ++nbadq;
        }
        // Stretches of lanes with one key: the lanes that hold a pixel are the first npx of the tile, so they are consecutive in the wave.
        const unsigned long long pkey = (unsigned long long)__shfl_up((long long)key, 1, 64);
        const bool first = have && (lane == 0 || pkey != key);
        const unsigned long long hv = __ballot(have);
        if (hv) {
            const unsigned long long stops = __ballot(first) | ~hv;              // lanes where a stretch begins, and lanes without a pixel
            unsigned long long pre = term;                                       // inclusive prefix sum over the wave
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long up = (unsigned long long)__shfl_up((long long)pre, d, 64);
                if (lane >= d) pre += up;
            }
            const unsigned long long above = lane == 63 ? 0ull : stops & ~((2ull << lane) - 1ull);
            const int last = above ? __ffsll((long long)above) - 2 : 63;         // the lane in front of the next stop: the end of this lane's stretch
            const unsigned long long pre_last = (unsigned long long)__shfl((long long)pre, last, 64);
            if (first) {
                const unsigned int cnt = (unsigned int)(last - lane + 1);
                const unsigned long long sum = pre_last - pre + term;
                if (!in_lds_insert(lk, lc, ls, key, cnt, sum) && !in_global_insert(tab, mask, limit, key, cnt, sum)) atomicOr(counts + 2, 1ull);
            }
        }
        if (S > 0) __syncthreads();                                              // the image is free for the next tile
    }
    if (nbad) atomicAdd(&s_bad, nbad);
    if (nbadq) atomicAdd(&s_badq, nbadq);
    __syncthreads();

    for (int i = t; i < IN_LSLOTS; i += IN_THREADS) {
        const unsigned long long key = lk[i];
        if (key != IN_EMPTY && !in_global_insert(tab, mask, limit, key, (unsigned long long)lc[i], ls[i])) atomicOr(counts + 2, 1ull);
    }
    if (t == 0 && s_bad) atomicAdd(counts + 1, (unsigned long long)s_bad);
    if (t == 0 && s_badq) atomicAdd(counts + 4, (unsigned long long)s_badq);
}

__global__ __launch_bounds__(IN_THREADS) void in_clear_kernel(unsigned long long* __restrict__ work, long long entries, unsigned long long* __restrict__ counts, int ncounts)
{
    const long long i = (long long)blockIdx.x * IN_THREADS + threadIdx.x;
    if (i < entries) {
        ulonglong2 e; e.x = IN_EMPTY; e.y = 0ull;
        reinterpret_cast<ulonglong2*>(work)[2 * i] = e;
        e.x = 0ull;
        reinterpret_cast<ulonglong2*>(work)[2 * i + 1] = e;
    }
    if (i < ncounts) counts[i] = 0ull;
}

// grid (slot blocks, N): a thread per slot
__global__ __launch_bounds__(IN_THREADS) void in_compact_kernel(const unsigned long long* __restrict__ work, unsigned int slots, long long* __restrict__ rows,
                                                                long long max_rows, unsigned long long* __restrict__ counts)
{
    __shared__ unsigned int s_rows;
    __shared__ unsigned long long s_pix, s_base;
    const int t = threadIdx.x, n = blockIdx.y, lane = t & 63;
    if (t == 0) { s_rows = 0u; s_pix = 0ull; }
    __syncthreads();
    const unsigned int s = blockIdx.x * IN_THREADS + t;
    unsigned long long key = IN_EMPTY, cnt = 0ull, sum = 0ull;
    if (s < slots) {
        const ulonglong2* e = reinterpret_cast<const ulonglong2*>(work) + 2 * ((size_t)n * slots + s);
        const ulonglong2 e0 = e[0], e1 = e[1];
        key = e0.x; cnt = e0.y; sum = e1.x;
    }
    const bool valid = key != IN_EMPTY;
    const unsigned long long ball = __ballot(valid);
    const unsigned int before = (unsigned int)__popcll(ball & ((1ull << lane) - 1ull));
    unsigned int wave_base = 0u;
    if (lane == 0 && ball) wave_base = atomicAdd(&s_rows, (unsigned int)__popcll(ball));
    wave_base = __shfl(wave_base, 0, 64);
    if (valid && cnt) atomicAdd(&s_pix, cnt);
    __syncthreads();
    if (t == 0) {
        s_base = s_rows ? atomicAdd(counts + 5 * (size_t)n, (unsigned long long)s_rows) : 0ull;
        if (s_pix) atomicAdd(counts + 5 * (size_t)n + 3, s_pix);
    }
    __syncthreads();
    if (valid) {
        const unsigned long long rank = s_base + wave_base + before;
        if (rank < (unsigned long long)max_rows) {
            long long* o = rows + ((size_t)n * (size_t)max_rows + rank) * 4;
            o[0] = (long long)(key >> 32); o[1] = (long long)(key & 0xFFFFFFFFull); o[2] = (long long)cnt; o[3] = (long long)sum;
        }
    }
}

size_t instance_work_bytes(int N, long long slots)
{
    if (N <= 0 || slots < 1 || slots > (1LL << 28) || (slots & (slots - 1))) return 0;
    return (size_t)N * (size_t)slots * 32;
}

void launch_instance_pair(const float* prob, int C, const uint8_t* labels, const int* comp, const uint16_t* inst, int N, int H, int W, void* work,
                          long long slots, long long* rows, long long max_rows, unsigned long long* counts, hipStream_t s)
{
    const long long P = (long long)H * W, entries = (long long)N * slots;
    const long long clear_items = entries > 5LL * N ? entries : 5LL * N;
    hipLaunchKernelGGL(in_clear_kernel, dim3((unsigned int)((clear_items + IN_THREADS - 1) / IN_THREADS)), dim3(IN_THREADS), 0, s,
                       (unsigned long long*)work, entries, counts, 5 * N);
    InArgs a = {};
    a.prob = prob; a.labels = labels; a.comp = comp; a.inst = inst; a.P = P; a.C = C;
    a.work = (unsigned long long*)work; a.slots = (unsigned int)slots; a.counts = counts;
    a.limit = (unsigned int)(slots >= 2 * P ? slots : (slots < IN_GPROBE ? slots : IN_GPROBE));
    // every image's rows start 16-byte aligned when the first does and a row is a multiple of 16 bytes
    bool vec = ((uintptr_t)prob & 15) == 0 && C % 4 == 0;
    int S = vec ? in_vec_stride(C) : (C & 1 ? C : C + 1);
    if (S > IN_MAX_STRIDE) { S = 0; vec = false; }
    a.S = S;
    // four blocks fit a CU beside each other at C = 20: at most one such round of the 256 CUs, every block of an image the same number of
    // trips, and at least IN_MIN_TRIPS of them where the image has that many tiles
    const long long tiles = (P + IN_THREADS - 1) / IN_THREADS;
    const long long target = N >= 1024 ? 1 : 1024 / N;
    long long trips = (tiles + target - 1) / target;
    if (trips < IN_MIN_TRIPS) trips = IN_MIN_TRIPS;
    const long long blocks = (tiles + trips - 1) / trips;
    const size_t lds = (size_t)IN_THREADS * S * 4;
    const dim3 grid((unsigned int)blocks, (unsigned int)N);
    if (vec && C == 20) hipLaunchKernelGGL((in_count_kernel<true, 20>), grid, dim3(IN_THREADS), lds, s, a);
    else if (vec) hipLaunchKernelGGL((in_count_kernel<true, 0>), grid, dim3(IN_THREADS), lds, s, a);
    else hipLaunchKernelGGL((in_count_kernel<false, 0>), grid, dim3(IN_THREADS), lds, s, a);
    hipLaunchKernelGGL(in_compact_kernel, dim3((unsigned int)((slots + IN_THREADS - 1) / IN_THREADS), (unsigned int)N), dim3(IN_THREADS), 0, s,
                       (const unsigned long long*)work, (unsigned int)slots, rows, max_rows, counts);
}

}  // namespace fcn8s
