// Class-balanced pseudo-labels from a softmax (fcn8s_op_pseudo_label; the definition is in fcn8s_hip.h): one pass over the N * P pixels of a
// batch that reads every input byte once (the softmax row 4 C B, the base label 1 B, the uncertainty 4 B), writes one label byte per pixel and
// feeds three integer tables: hist [C][1024], counts [C][2], misc [3].  Integers only: the result does not depend on the order in which
// pixels arrive.
//
// Loads.  The tile scheme of reliability.hip, restated here.  The batch is one flat run of N * P rows of C floats.  A block of 256 threads
// takes a tile of 256 consecutive pixels per trip: the tile's 256 C floats are brought in with lane-contiguous loads (16 bytes per lane when the
// base pointer is 16-byte aligned and C % 4 == 0: a wave's load is then 1 KiB of consecutive bytes whatever C is; 4 bytes per lane otherwise),
// written to an LDS image [256][S] and read back one row per thread.  The row stride S (in floats) is chosen so that the row reads do not
// conflict:
//   16-byte path  S = C if C / 4 is odd, else C + 4: rows are read with ds_read_b128, whose 16 lanes of a group then start on 16 different
//                 16-byte slots of the 256-byte bank row.  For C = 20, S = 20: the image is the tile itself.
//   generic path  S = C if C is odd, else C + 1: rows are read with ds_read_b32 at an odd stride, 32 lanes on 32 banks.
// With C == 20 on the 16-byte path the next tile's loads (five 16-byte loads, the base byte and the score) are issued into registers before the
// current tile is counted.  A row stride of more than 64 floats does not fit the image: such C read their rows from global memory, a thread
// per row (correct, not fast).
//
// Labels.  A thread puts its pixel's byte into an LDS strip at the offset the tile's first byte has inside its 16-byte line of global memory,
// so that 16-byte pieces of the strip are 16-byte lines of labels_out.  After the tile's barrier the first 17 threads write one line each: a
// line that lies inside the tile leaves as one 16-byte store, the two ragged ones (the first when labels_out is not 16-byte aligned, the last
// of the batch) as byte stores.  No byte outside the N * P labels is written.
//
// Counting.  Block-private LDS tables, one global 64-bit atomic per non-zero entry at block end.
//   hist    The full table of 32-bit counters is 4 KB per class -- 80 KB at C = 20, one block of 4 waves per CU next to the 20 KB image.  This
//           is a streaming kernel: what hides HBM latency is the bytes in flight per CU (about 32 KiB), here the next tile of every wave,
//           5 KiB each, and 4 waves hold 20 KiB (not measured apart: with the slots below, one block per CU also flushes less).  Direct global
//           atomics cost one 64-bit atomic per pixel on a handful of cache lines (a trained model puts most pixels of a class into the
//           last bins).  So the table is the third form: PL_SLOTS = 2048 open-addressed slots {key = k * 1024 + b, count} in 16 KB, as
//           panoptic.hip keys its pairs: 38.6 KB per block at C = 20.  A trained model touches about a thousand keys per block; 2048 hold
//           every key of a block that meets fewer than that many distinct ones.  A key that finds neither itself nor a free slot within
//           PL_PROBES probes goes to global memory with one atomic of its own (the spill; uniform random softmaxes over many tiles reach
//           it, and it is the same count by another way -- and the slow one: see the README's figures).  The slots take any C up to 255.
//           Within a wave pl_wave_share aggregates first: where a lane's left neighbour holds the same index (one DPP move, one ballot) the
//           first such lane becomes leader and adds the pop-count of the lanes that share its index with ONE atomic; the lanes left add
//           their own 1.  Any arrangement of lanes gives the same counts.
//           Flush.  Up to PL_FLUSH_KEYS keys (C <= 32) a block walks the KEYS and looks each up in its slots, so that a wave's 64 atomics lie
//           in four cache lines of the global table.  Walking the slots scatters them over 64 lines, and the about 80 hot lines of a
//           trained model's table then take every atomic of every block one after the other: 351 us against 171 us for the whole kernel at
//           16 x 1024 x 512 x 20.
//   blocks  PL_BLOCKS_PER_CU = 2, 8 waves and 40 KiB of loads in flight per CU.  Measured against 4 (the neighbours' cap): the label modes
//           take the same time at 16 x 1024 x 512 and 41 against 47 us at 1 x 2048 x 1024, and the histogram mode 159 against 171 us on
//           trained-like input -- half as many blocks are half as many flushes into the same hot lines.
//   counts  [C][2] 32-bit LDS counters through the same wave aggregation (index 2 k + dropped).
//   misc    per-thread 64-bit registers over the block's trips, one wave reduction at block end.
// Every loop is bounded (PL_PROBES probes, the grid-stride loop); no block waits for another; there is no ticket and no fence.
// Overflow bound of the 32-bit LDS entries: a block sees at most 2^23 tiles of 256 pixels (the launcher raises the grid when N * P asks for it).
#include "fcn8s_internal.h"

namespace fcn8s {

#define PL_THREADS FCN8S_PL_TILE_PIXELS
#define PL_M FCN8S_PL_BINS
#define PL_MAX_STRIDE 64                             // floats per row of the LDS image: 64 KB for the tile
#define PL_MAX_TRIPS (1LL << 23)
#define PL_SLOTS 2048                                // a power of two
#define PL_SLOT_SHIFT 21                             // 32 - log2(PL_SLOTS)
#define PL_PROBES 8
#define PL_BLOCKS_PER_CU 2                            // the header comment has the measurement
#define PL_FLUSH_KEYS 32768                          // up to this many keys (C <= 32) the flush walks the keys, beyond it the slots
#define PL_EMPTY 0xFFFFFFFFu                         // no key: the largest one is 254 * 1024 + 1023
#define PL_STRIP (PL_THREADS + 16)                   // the label strip: the tile behind an offset of 0 .. 15 bytes
#define PL_LINES (PL_STRIP / 16)

struct PlArgs {
    const float* prob; const float* thr; const uint8_t* oid; const uint8_t* base; const float* score;
    uint8_t* labels;
    long long T;                                     // N * P
    int C, S;                                        // S: row stride of the LDS image in floats, 0 = rows are read from global memory
    unsigned int ignore_id, base_fill;
    float score_max;
    unsigned long long *hist, *counts, *misc;
};

// row stride of the LDS image on the 16-byte path (the header comment has the rule)
__host__ __device__ constexpr int pl_vec_stride(int C) { return (C / 4) & 1 ? C : C + 4; }

// what a thread holds of a tile before it is counted: its base byte and score, and (NV > 0) its NV 16-byte pieces of the tile's rows
template <int NV>
struct PlIn {
    float4 pv[NV > 0 ? NV : 1];
    unsigned int b;
    float s;
};

template <int NV>
__device__ __forceinline__ void pl_load(const PlArgs& a, long long tile, int t, PlIn<NV>& in)
{
    const long long g0 = tile * PL_THREADS;
    const long long left = a.T - g0;
    const int npx = left < PL_THREADS ? (int)left : PL_THREADS;
    if (NV > 0) {
        const float4* src = reinterpret_cast<const float4*>(a.prob + g0 * (NV * 4));
        const int nvec = npx * NV;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = t + k * PL_THREADS;
            in.pv[k] = i < nvec ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    in.b = a.base_fill; in.s = 0.f;
    if (t < npx) {
        if (a.base) in.b = a.base[g0 + t];
        if (a.score) in.s = a.score[g0 + t];
    }
}

// One row: k = argmax (lowest index on ties; c replaces the running maximum only if p_c > it), conf = p_k.
template <bool VEC, int CT>
__device__ __forceinline__ void pl_row(const float* __restrict__ row, int C, float& conf, int& best)
{
    float bv = 0.f; int bi = 0;
    if (VEC) {
        const float4* r4 = reinterpret_cast<const float4*>(__builtin_assume_aligned(row, 16));
        const int n4 = CT > 0 ? CT / 4 : C / 4;
#pragma unroll
        for (int i = 0; i < n4; ++i) {
            const float4 q = r4[i];
            const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = 4 * i + j;
                if (c == 0 || v[j] > bv) { bv = v[j]; bi = c; }
            }
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const float v = row[c];
            if (c == 0 || v > bv) { bv = v; bi = c; }
        }
    }
    conf = bv; best = bi;
}

// What this lane is to add at idx so that, over the wave, every lane with `on` has added 1 (the header comment has the rule): the pop-count
// for a leader, 0 for the lanes it speaks for, 1 for the others.  Called by all lanes of a wave together.
__device__ __forceinline__ unsigned int pl_wave_share(bool on, unsigned int idx, int lane)
{
    // the index of the lane to the left (row_shr:1; the first lane of a row of 16 sees ~0, which is no index)
    const unsigned int left = (unsigned int)__builtin_amdgcn_update_dpp(-1, (int)idx, 0x111, 0xf, 0xf, false);
    const unsigned long long pairs = __ballot(on && left == idx);
    unsigned int n = on ? 1u : 0u;
    if (pairs) {
        const int leader = __ffsll((long long)pairs) - 1;
        const unsigned int lead = (unsigned int)__builtin_amdgcn_readlane((int)idx, leader);
        const unsigned long long same = __ballot(on && idx == lead);
        if (on && idx == lead) n = lane == leader ? (unsigned int)__popcll(same) : 0u;
    }
    return n;
}

// hist[key] += n through the block's slots; at most PL_PROBES probes, then the global table itself
__device__ __forceinline__ void pl_hist_add(unsigned int* keys, unsigned int* cnt, unsigned long long* ghist, unsigned int key, unsigned int n)
{
    const unsigned int h = (key * 2654435761u) >> PL_SLOT_SHIFT;
#pragma unroll 1
    for (int probe = 0; probe < PL_PROBES; ++probe) {
        const unsigned int slot = (h + (unsigned int)probe) & (PL_SLOTS - 1);
        unsigned int seen = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (seen == PL_EMPTY) seen = atomicCAS(&keys[slot], PL_EMPTY, key);
        if (seen == PL_EMPTY || seen == key) { atomicAdd(&cnt[slot], n); return; }
    }
    atomicAdd(&ghist[key], (unsigned long long)n);
}

__device__ __forceinline__ unsigned long long pl_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned long long)__shfl_down((long long)v, d, 64);
    return v;
}

// grid: blocks (<= tiles), block: PL_THREADS.  VEC: the 16-byte path; CT: C as a compile-time constant (next-tile loads in registers), 0 = a.C
template <bool VEC, int CT>
__global__ __launch_bounds__(PL_THREADS) void pseudo_label_kernel(const PlArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long pl_lds[];
    constexpr int NV = CT / 4;
    const int t = threadIdx.x, lane = t & 63;
    const int C = CT > 0 ? CT : a.C, S = CT > 0 ? pl_vec_stride(CT) : a.S;
    unsigned long long* red = pl_lds;                                                           // [4]
    unsigned int* keys = reinterpret_cast<unsigned int*>(red + 4);                              // [PL_SLOTS]
    unsigned int* cnt = keys + PL_SLOTS;                                                        // [PL_SLOTS]
    float* thr = reinterpret_cast<float*>(cnt + PL_SLOTS);                                      // [256]
    uint8_t* oid = reinterpret_cast<uint8_t*>(thr + 256);                                       // [256]
    uint8_t* strip = oid + 256;                                                                 // [PL_STRIP]
    unsigned int* kd = reinterpret_cast<unsigned int*>(strip + PL_STRIP);                       // [C][2], padded to a multiple of 4 entries
    float* stage = reinterpret_cast<float*>(kd + ((2 * C + 3) & ~3));                           // [PL_THREADS][S]: every offset a multiple of 16 bytes
    const bool with_hist = a.hist != nullptr, with_labels = a.labels != nullptr;
    for (int i = t; i < PL_SLOTS; i += PL_THREADS) { keys[i] = PL_EMPTY; cnt[i] = 0u; }
    for (int i = t; i < 2 * C; i += PL_THREADS) kd[i] = 0u;
    if (t < 4) red[t] = 0ull;
    thr[t] = (a.thr && t < C) ? a.thr[t] : 0.f;                                                 // PL_THREADS == 256 entries
    oid[t] = (a.oid && t < C) ? a.oid[t] : (uint8_t)t;
    __syncthreads();

    const long long tiles = (a.T + PL_THREADS - 1) / PL_THREADS;
    const int shift = with_labels ? (int)((uintptr_t)a.labels & 15) : 0;                        // a tile starts at a multiple of 256 bytes of labels_out
    unsigned long long n_bad = 0, n_pass = 0, n_score = 0;
    PlIn<NV> in;
    if ((long long)blockIdx.x < tiles) pl_load<NV>(a, blockIdx.x, t, in);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long g0 = tile * PL_THREADS;
        const long long left = a.T - g0;
        const int npx = left < PL_THREADS ? (int)left : PL_THREADS;
        if (S > 0) {
            if (NV > 0) {
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int f = (t + k * PL_THREADS) * 4, px = f / C, c = f - px * C;         // px < 256 for every k < NV
                    *reinterpret_cast<float4*>(stage + px * S + c) = in.pv[k];
                }
            } else if (VEC) {
                const float4* src = reinterpret_cast<const float4*>(a.prob + g0 * C);
                const int nvec = npx * (C / 4);
                for (int i = t; i < nvec; i += PL_THREADS) {
                    const int f = i * 4, px = f / C, c = f - px * C;
                    *reinterpret_cast<float4*>(stage + px * S + c) = src[i];
                }
            } else {
                const float* src = a.prob + g0 * C;
                const int nfl = npx * C, dq = PL_THREADS / C, dr = PL_THREADS % C;
                int px = t / C, c = t - px * C;
                for (int i = t; i < nfl; i += PL_THREADS) {
                    stage[px * S + c] = src[i];
                    px += dq; c += dr;
                    if (c >= C) { c -= C; ++px; }
                }
            }
        }
        __syncthreads();                                                                        // the image is filled; the strip's lines of the tile before have left
        const unsigned int bv = in.b;
        const float sv = in.s;
        const long long next = tile + gridDim.x;
        if (next < tiles) pl_load<NV>(a, next, t, in);                                         // in flight while this tile is counted

        unsigned int lab = a.ignore_id, hkey = PL_EMPTY, kidx = PL_EMPTY;
        bool h_on = false, k_on = false;
        if (t < npx) {
            if (bv != a.base_fill) {
                lab = bv; ++n_pass;
            } else {
                const float* row = S > 0 ? stage + t * S : a.prob + (g0 + t) * C;
                float conf; int k;
                pl_row<VEC, CT>(row, C, conf, k);
                if (!isfinite(conf)) {
                    ++n_bad;
                } else if (a.score && !(sv <= a.score_max)) {
                    ++n_score; k_on = true; kidx = (unsigned int)k * 2u + 1u;
                } else {
                    const float x = conf * (float)PL_M;
                    const int b = x >= (float)PL_M ? PL_M - 1 : (conf > 0.f ? (int)x : 0);
                    h_on = with_hist; hkey = (unsigned int)k * PL_M + (unsigned int)b;
                    const bool keep = conf >= thr[k];
                    k_on = true; kidx = (unsigned int)k * 2u + (keep ? 0u : 1u);
                    if (keep) lab = oid[k];
                }
            }
        }
        if (with_hist) {
            const unsigned int n = pl_wave_share(h_on, h_on ? hkey : PL_EMPTY, lane);
            if (n) pl_hist_add(keys, cnt, a.hist, hkey, n);
        }
        {
            const unsigned int n = pl_wave_share(k_on, kidx, lane);
            if (n) atomicAdd(&kd[kidx], n);
        }
        if (with_labels && t < npx) strip[shift + t] = (uint8_t)lab;
        __syncthreads();                                                                        // the image is free for the next tile; the strip is whole
        if (with_labels && t < PL_LINES) {
            const int lo = t * 16, first = shift, last = shift + npx;                           // the strip's bytes [first, last) are the tile's labels
            uint8_t* line = a.labels + g0 + (lo - shift);                                      // a 16-byte line of global memory; only its bytes inside the tile are touched
            if (lo >= first && lo + 16 <= last) {
                *reinterpret_cast<uint4*>(line) = *reinterpret_cast<const uint4*>(strip + lo);
            } else {
                const int i0 = lo > first ? lo : first, i1 = lo + 16 < last ? lo + 16 : last;
                for (int i = i0; i < i1; ++i) line[i - lo] = strip[i];
            }
        }
    }

    unsigned long long r[3] = {n_bad, n_pass, n_score};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r[i] = pl_wave_sum(r[i]);
        if (lane == 0 && r[i]) atomicAdd(&red[i], r[i]);
    }
    __syncthreads();
    // blocks end at about the same time: each starts its flush at another piece of its slots, so that they do not all queue on the same addresses
    const int nkeys = C * PL_M;
    if (with_hist && nkeys <= PL_FLUSH_KEYS) {
        // in key order: the slots are looked up, not walked, so that a wave's 64 atomics lie in four cache lines of the table, as a direct
        // table's would (walked in slot order they lie in 64, and the few hot lines of a trained model's table take every one of them in turn)
        const int k0 = (int)(((long long)blockIdx.x * PL_THREADS) % nkeys);
        for (int i = t; i < nkeys; i += PL_THREADS) {
            const unsigned int key = (unsigned int)(i + k0 < nkeys ? i + k0 : i + k0 - nkeys);
            const unsigned int h = (key * 2654435761u) >> PL_SLOT_SHIFT;
            unsigned int v = 0u;
#pragma unroll 1
            for (int probe = 0; probe < PL_PROBES; ++probe) {                                   // an insert stopped at the key or at the first free slot
                const unsigned int slot = (h + (unsigned int)probe) & (PL_SLOTS - 1);
                const unsigned int seen = keys[slot];
                if (seen == key) v = cnt[slot];
                if (seen == key || seen == PL_EMPTY) break;
            }
            if (v) atomicAdd(&a.hist[key], (unsigned long long)v);
        }
    } else if (with_hist) {
        const int h0 = (int)(((long long)blockIdx.x * PL_THREADS) % PL_SLOTS);
        for (int i = t; i < PL_SLOTS; i += PL_THREADS) {
            const int e = (i + h0) & (PL_SLOTS - 1);
            if (keys[e] != PL_EMPTY && cnt[e]) atomicAdd(&a.hist[keys[e]], (unsigned long long)cnt[e]);
        }
    }
    for (int i = t; i < 2 * C; i += PL_THREADS)
        if (kd[i]) atomicAdd(&a.counts[i], (unsigned long long)kd[i]);
    if (t < 3 && red[t]) atomicAdd(&a.misc[t], red[t]);
}

template <bool VEC, int CT>
static bool pl_launch(const PlArgs& a, int blocks, size_t lds, hipStream_t s)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pseudo_label_kernel<VEC, CT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "pseudo_label: %zu bytes of LDS refused (%s)", lds, hipGetErrorString(e)); return false; }
    }
    hipLaunchKernelGGL((pseudo_label_kernel<VEC, CT>), dim3(blocks), dim3(PL_THREADS), lds, s, a);
    return true;
}

void launch_pseudo_label(const float* prob, int N, long long P, int C, const float* thresholds, const uint8_t* out_ids, int ignore_id,
                         const uint8_t* base, int base_fill, const float* score, float score_max, uint8_t* labels_out,
                         unsigned long long* hist, unsigned long long* counts, unsigned long long* misc, hipStream_t s)
{
    PlArgs a = {};
    a.prob = prob; a.thr = thresholds; a.oid = out_ids; a.base = base; a.score = score; a.labels = labels_out;
    a.T = (long long)N * P; a.C = C;
    a.ignore_id = (unsigned int)ignore_id; a.base_fill = (unsigned int)base_fill; a.score_max = score_max;
    a.hist = hist; a.counts = counts; a.misc = misc;
    bool vec = ((uintptr_t)prob & 15) == 0 && C % 4 == 0;
    int S = vec ? pl_vec_stride(C) : (C & 1 ? C : C + 1);
    if (S > PL_MAX_STRIDE) { S = 0; vec = false; }
    a.S = S;
    const long long tiles = (a.T + PL_THREADS - 1) / PL_THREADS;
    long long blocks = tiles < FCN8S_PL_MAX_BLOCKS ? tiles : FCN8S_PL_MAX_BLOCKS;
    const size_t lds = 32 + (size_t)PL_SLOTS * 8 + 256 * 4 + 256 + PL_STRIP + (size_t)((2 * C + 3) & ~3) * 4 + (size_t)PL_THREADS * S * 4;
    // no more blocks than are resident at once (256 CUs, 160 KB of LDS each, at most PL_BLOCKS_PER_CU blocks per CU): a second, partly filled
    // round of blocks costs more than longer loops do, and every block ends with its own flush
    long long per_cu = (long long)(160 * 1024 / lds);
    per_cu = per_cu > PL_BLOCKS_PER_CU ? PL_BLOCKS_PER_CU : (per_cu < 1 ? 1 : per_cu);
    if (blocks > 256 * per_cu) blocks = 256 * per_cu;
    const long long need = (tiles + PL_MAX_TRIPS - 1) / PL_MAX_TRIPS;
    if (blocks < need) blocks = need;
    if (vec && C == 20) pl_launch<true, 20>(a, (int)blocks, lds, s);
    else if (vec) pl_launch<true, 0>(a, (int)blocks, lds, s);
    else pl_launch<false, 0>(a, (int)blocks, lds, s);
}

}  // namespace fcn8s
