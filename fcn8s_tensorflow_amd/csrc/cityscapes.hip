// Cityscapes pixel-level scoring counts (fcn8s_op_cityscapes_pair; the definition is in fcn8s_hip.h): one pass over a batch of N
// same-size images that reads every input byte once (ground-truth label ids 1 B, instance ids 2 B, prediction 8 B as the int64 train
// ids `predict` returns or 1 B as label ids) and feeds
//   * the 34 x 34 confusion matrix conf[gt, pred],
//   * per instance value v (> 1000, label v / 1000 counted) the three counts size / tp / cattp,
//   * the two error counters (pixels with an id out of range, pixels of a value v the evaluator cannot score),
// followed by an ordered compaction of the per-image count table into entries {v, size, tp, cattp}, ascending v (a second, small kernel:
// doing it in the counting kernel's last block per image needs agent-scope fences in every block, whose L2 write-back and invalidate made
// the pass four times slower when measured).
// Integers only: the result does not depend on the order in which pixels arrive.
//
// Counter design.  A lane owns 16 consecutive pixels of one image (one 16-byte load of gt, two of the instance map, eight of an int64
// prediction) and folds them into runs of equal (v, gt, pred) in registers: label and instance ids are constant over long stretches of a
// row, so a run usually spans all 16 pixels.  Each run costs one 32-bit LDS atomic into the block's private 34 x 34 histogram and, when
// v is a counted instance, ONE 64-bit LDS atomic into the block's private instance table (8 labels x 1000 ids, 64 KB), which packs the
// three counts of that run as size | tp << 21 | cattp << 42.  Noise (every pixel a run of its own) degrades to the one-LDS-atomic-per-
// pixel of confusion_kernel plus one more for instance pixels; global memory sees one atomic per non-zero bin per block at the end.
//   Overflow bound of the packing: a field holds at most the pixels ONE BLOCK sees of one image.  The launcher gives a block at most
// CS_MAX_CHUNKS chunks of CS_CHUNK pixels plus (block 0) the < 16 pixels in front of the first aligned one:
// 255 * 8192 + 15 = 2088975 < 2^21 = 2097152, so no field carries into its neighbour; the 32-bit histogram bins are bounded by the same
// figure.  The per-image table in global memory is 32 bits per count and entries are int32: P < 2^31 pixels per image, larger images are
// refused with FCN8S_ERR_SHAPE by the entry point.  conf is 64 bits.
#include "fcn8s_internal.h"

namespace fcn8s {

#define CS_THREADS 512
#define CS_PIX 16                                    // pixels per lane per trip
#define CS_CHUNK (CS_THREADS * CS_PIX)               // 8192 pixels per block per trip
#define CS_MAX_CHUNKS 255                            // per block: see the overflow bound above
#define CS_IDS 34
#define CS_SLOTS 8000                                // 8 counted instance labels x ids 0..999
#define CS_BADKEY 0xFFFFFFFFu

__device__ __forceinline__ unsigned int cs_train_to_label(unsigned int t)       // labels.py trainId -> id, t < 20
{
    // bytes: 0,7,8,11,12,13,17,19 | 20,21,22,23,24,25,26,27 | 28,31,32,33
    const unsigned long long w = t < 8 ? 0x13110D0C0B080700ull : (t < 16 ? 0x1B1A191817161514ull : 0x0000000021201F1Cull);
    return (unsigned int)(w >> ((t & 7) * 8)) & 0xFFu;
}
// label of an instance value: 1 = counted (person, rider, car, truck, bus, train, motorcycle, bicycle), 0 = ignoreInEval (skipped),
// 2 = an evaluated label without instances or no label at all (the evaluator's KeyError)
__device__ __forceinline__ int cs_label_kind(unsigned int L)
{
    if (L >= CS_IDS) return 2;
    const unsigned long long counted = 0x39F000000ull;                           // bits 24..28, 31..33
    const unsigned long long skipped = 0x06005C67Full;                           // bits 0..6, 9, 10, 14, 15, 16, 18, 29, 30
    return (counted >> L) & 1 ? 1 : ((skipped >> L) & 1 ? 0 : 2);
}

template <bool INST>
__device__ __forceinline__ void cs_flush(unsigned int key, unsigned int n, unsigned int* hist, unsigned long long* tab,
                                         unsigned int& nbad, unsigned int& nbadv)
{
    if (n == 0) return;
    if (key == CS_BADKEY) { nbad += n; return; }
    const unsigned int lab = key & 0xFFu, g = (key >> 8) & 0xFFu;
    atomicAdd(&hist[g * CS_IDS + lab], n);
    if (INST) {
        const unsigned int v = key >> 16;
        if (v > 1000u) {
            const unsigned int L = v / 1000u;
            const int kind = cs_label_kind(L);
            if (kind == 1) {
                const unsigned int slot = (L <= 28u ? L - 24u : L - 26u) * 1000u + (v - L * 1000u);
                const bool incat = L <= 25u ? (lab == 24u || lab == 25u) : (lab >= 26u && lab <= 33u);     // human | vehicle (29, 30 included)
                unsigned long long add = n;
                if (lab == L) add |= (unsigned long long)n << 21;
                if (incat) add |= (unsigned long long)n << 42;
                atomicAdd(&tab[slot], add);
            } else if (kind == 2) {
                nbadv += n;
            }
        }
    }
}

// 16 (or, at an image's ends and on unaligned buffers, m < 16 scalar-loaded) consecutive pixels starting at pixel q of the image
template <bool INST, int KIND>
__device__ __forceinline__ void cs_group(const uint8_t* __restrict__ gt, const uint16_t* __restrict__ inst, const void* __restrict__ pred,
                                         long long q, int m, bool vec, unsigned int* hist, unsigned long long* tab,
                                         unsigned int& nbad, unsigned int& nbadv)
{
    unsigned int g[CS_PIX], v[CS_PIX], lab[CS_PIX];
    if (vec) {
        const uint4 gw = *reinterpret_cast<const uint4*>(gt + q);
        const unsigned int gws[4] = {gw.x, gw.y, gw.z, gw.w};
#pragma unroll
        for (int i = 0; i < CS_PIX; ++i) g[i] = (gws[i >> 2] >> ((i & 3) * 8)) & 0xFFu;
        if (INST) {
            const uint4 a = *reinterpret_cast<const uint4*>(inst + q), b = *reinterpret_cast<const uint4*>(inst + q + 8);
            const unsigned int vs[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < CS_PIX; ++i) v[i] = (vs[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu;
        }
        if (KIND == 0) {
            const uint4* pp = reinterpret_cast<const uint4*>(reinterpret_cast<const long long*>(pred) + q);
            uint4 pw[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) pw[i] = pp[i];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                lab[2 * i] = (pw[i].y == 0u && pw[i].x < 20u) ? cs_train_to_label(pw[i].x) : 255u;
                lab[2 * i + 1] = (pw[i].w == 0u && pw[i].z < 20u) ? cs_train_to_label(pw[i].z) : 255u;
            }
        } else {
            const uint4 pw = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(pred) + q);
            const unsigned int pws[4] = {pw.x, pw.y, pw.z, pw.w};
#pragma unroll
            for (int i = 0; i < CS_PIX; ++i) lab[i] = (pws[i >> 2] >> ((i & 3) * 8)) & 0xFFu;
        }
    } else {
#pragma unroll
        for (int i = 0; i < CS_PIX; ++i) {
            g[i] = 255u; v[i] = 0u; lab[i] = 255u;
            if (i < m) {
                g[i] = gt[q + i];
                if (INST) v[i] = inst[q + i];
                if (KIND == 0) {
                    const unsigned long long t = (unsigned long long)reinterpret_cast<const long long*>(pred)[q + i];
                    lab[i] = t < 20ull ? cs_train_to_label((unsigned int)t) : 255u;
                } else {
                    lab[i] = reinterpret_cast<const uint8_t*>(pred)[q + i];
                }
            }
        }
    }
    unsigned int cur = CS_BADKEY, n = 0;
#pragma unroll
    for (int i = 0; i < CS_PIX; ++i) {
        if (i < m) {
            const unsigned int key = (g[i] >= CS_IDS || lab[i] >= CS_IDS) ? CS_BADKEY : ((INST ? v[i] << 16 : 0u) | g[i] << 8 | lab[i]);
            if (key == cur) { ++n; }
            else { cs_flush<INST>(cur, n, hist, tab, nbad, nbadv); cur = key; n = 1; }
        }
    }
    cs_flush<INST>(cur, n, hist, tab, nbad, nbadv);
}

// grid (blocks per image, N).  work: [N][CS_SLOTS] uint4 {size, tp, cattp, -}; errs_out + n * err_stride: the image's two error counters
// (inside work behind the tables when there is an instance map, counts[n][1..2] otherwise); all of it zeroed by the launcher.
template <bool INST, int KIND>
__global__ __launch_bounds__(CS_THREADS) void cityscapes_count_kernel(const uint8_t* __restrict__ gt_all, const uint16_t* __restrict__ inst_all,
                                                                      const void* __restrict__ pred_all, long long P, int vec_ok,
                                                                      unsigned long long* __restrict__ conf, unsigned int* __restrict__ work,
                                                                      unsigned long long* __restrict__ errs_out, int err_stride)
{
    extern __shared__ unsigned long long cs_lds[];
    unsigned long long* tab = cs_lds;                                                        // [CS_SLOTS] (INST only)
    unsigned int* hist = reinterpret_cast<unsigned int*>(cs_lds + (INST ? CS_SLOTS : 0));    // [34 * 34]
    unsigned int* errs = hist + CS_IDS * CS_IDS;                                             // [2]
    const int t = threadIdx.x, n = blockIdx.y;
    if (INST) for (int i = t; i < CS_SLOTS; i += CS_THREADS) tab[i] = 0ull;
    for (int i = t; i < CS_IDS * CS_IDS + 2; i += CS_THREADS) hist[i] = 0u;
    __syncthreads();

    const long long base = (long long)n * P;
    const uint8_t* gt = gt_all + base;
    const uint16_t* inst = INST ? inst_all + base : nullptr;
    const void* pred = KIND == 0 ? (const void*)(reinterpret_cast<const long long*>(pred_all) + base)
                                 : (const void*)(reinterpret_cast<const uint8_t*>(pred_all) + base);
    // the buffers are 16-byte aligned (vec_ok), so pixel `base + head` is the image's first one on a 16-byte boundary of all three maps
    long long head = vec_ok ? (16 - (base & 15)) & 15 : 0;
    if (head > P) head = P;
    const long long body = P - head;
    const long long nchunks = (body + CS_CHUNK - 1) / CS_CHUNK;
    unsigned int nbad = 0, nbadv = 0;
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long long q = head + c * CS_CHUNK + (long long)t * CS_PIX;
        const long long left = P - q;
        if (left >= CS_PIX && vec_ok) cs_group<INST, KIND>(gt, inst, pred, q, CS_PIX, true, hist, tab, nbad, nbadv);
        else if (left > 0) cs_group<INST, KIND>(gt, inst, pred, q, left < CS_PIX ? (int)left : CS_PIX, false, hist, tab, nbad, nbadv);
    }
    if (blockIdx.x == 0 && t == 0 && head > 0) cs_group<INST, KIND>(gt, inst, pred, 0, (int)head, false, hist, tab, nbad, nbadv);
    if (nbad) atomicAdd(&errs[0], nbad);
    if (nbadv) atomicAdd(&errs[1], nbadv);
    __syncthreads();

    for (int i = t; i < CS_IDS * CS_IDS; i += CS_THREADS)
        if (hist[i]) atomicAdd(&conf[i], (unsigned long long)hist[i]);
    if (t < 2 && errs[t]) atomicAdd(&errs_out[(size_t)n * err_stride + t], (unsigned long long)errs[t]);
    if (INST) {
        unsigned int* w = work + (size_t)n * CS_SLOTS * 4;
        for (int i = t; i < CS_SLOTS; i += CS_THREADS) {
            const unsigned long long p = tab[i];
            if (p) {
                const unsigned int size = (unsigned int)(p & 0x1FFFFFull), tp = (unsigned int)((p >> 21) & 0x1FFFFFull), cattp = (unsigned int)(p >> 42);
                atomicAdd(&w[i * 4], size);
                if (tp) atomicAdd(&w[i * 4 + 1], tp);
                if (cattp) atomicAdd(&w[i * 4 + 2], cattp);
            }
        }
    }
}

// One block of 1024 threads per image: thread t owns slots 8t .. 8t+7 (ascending v), counts the occupied ones, an exclusive scan over
// the block gives each its rank; entries[n][rank] = {v, size, tp, cattp} for rank < max_entries, counts[n] = {number of occupied slots, the two
// error counters of the counting pass}.
__global__ __launch_bounds__(1024) void cityscapes_compact_kernel(const unsigned int* __restrict__ work, const unsigned long long* __restrict__ errs,
                                                                  int* __restrict__ entries, int max_entries, unsigned long long* __restrict__ counts)
{
    __shared__ unsigned int wave_sum[16];
    const int t = threadIdx.x, n = blockIdx.x, lane = t & 63, wv = t >> 6;
    const uint4* w = reinterpret_cast<const uint4*>(work) + (size_t)n * CS_SLOTS;
    uint4 e[8];
    unsigned int mine = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int slot = t * 8 + i;
        e[i] = slot < CS_SLOTS ? w[slot] : make_uint4(0, 0, 0, 0);
        mine += e[i].x != 0u;
    }
    unsigned int incl = mine;                                  // inclusive scan within the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wv] = incl;
    __syncthreads();
    unsigned int before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) { const unsigned int s = wave_sum[i]; if (i < wv) before += s; total += s; }
    unsigned int rank = before + incl - mine;
    int* out = entries + (size_t)n * max_entries * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (e[i].x != 0u) {
            if (rank < (unsigned int)max_entries) {
                const int slot = t * 8 + i, ci = slot / 1000, L = ci < 5 ? 24 + ci : 26 + ci;
                int* o = out + (size_t)rank * 4;
                o[0] = L * 1000 + (slot - ci * 1000); o[1] = (int)e[i].x; o[2] = (int)e[i].y; o[3] = (int)e[i].z;
            }
            ++rank;
        }
    }
    if (t == 0) { counts[n * 3] = total; counts[n * 3 + 1] = errs[n * 2]; counts[n * 3 + 2] = errs[n * 2 + 1]; }
}

// [N][CS_SLOTS] uint4 tables, then [N][2] 64-bit error counters: cleared by ONE memset per call
size_t cityscapes_work_bytes(int N) { return N > 0 ? (size_t)N * (CS_SLOTS * 16 + 16) : 0; }

template <bool INST, int KIND>
static bool cs_launch_count(const uint8_t* gt, const uint16_t* inst, const void* pred, int N, long long P, int vec_ok, int blocks,
                            unsigned long long* conf, unsigned int* work, unsigned long long* errs_out, int err_stride, hipStream_t s)
{
    const size_t lds = (INST ? (size_t)CS_SLOTS * 8 : 0) + (CS_IDS * CS_IDS + 2) * sizeof(unsigned int);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cityscapes_count_kernel<INST, KIND>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "cityscapes_pair: %zu bytes of LDS refused (%s)", lds, hipGetErrorString(e)); return false; }
    }
    hipLaunchKernelGGL((cityscapes_count_kernel<INST, KIND>), dim3(blocks, N), dim3(CS_THREADS), lds, s, gt, inst, pred, P, vec_ok, conf, work, errs_out, err_stride);
    return true;
}

void launch_cityscapes_pair(const uint8_t* gt, const uint16_t* inst, const void* pred, int pred_kind, int N, long long P,
                            unsigned long long* conf, void* work, int* entries, int max_entries, unsigned long long* counts, hipStream_t s)
{
    if ((inst ? hipMemsetAsync(work, 0, cityscapes_work_bytes(N), s) : hipMemsetAsync(counts, 0, (size_t)N * 3 * sizeof(unsigned long long), s)) != hipSuccess) {
        defer_error(FCN8S_ERR_HIP, "cityscapes_pair: clearing the counters failed"); return;
    }
    // two blocks of 512 threads fit a CU beside each other (69 KB of LDS each): one such round of the 256 CUs, never more than
    // CS_MAX_CHUNKS chunks per block (the packing's overflow bound), never more blocks than chunks
    const long long nchunks = (P + CS_CHUNK - 1) / CS_CHUNK;
    long long blocks = (512 + N - 1) / N;
    const long long need = (nchunks + CS_MAX_CHUNKS - 1) / CS_MAX_CHUNKS;
    if (blocks < need) blocks = need;
    if (blocks > nchunks) blocks = nchunks;
    const int vec_ok = (((uintptr_t)gt | (uintptr_t)inst | (uintptr_t)pred) & 15) == 0;
    if (inst) {
        unsigned long long* errs = reinterpret_cast<unsigned long long*>(static_cast<char*>(work) + (size_t)N * CS_SLOTS * 16);
        const bool ok = pred_kind == 0 ? cs_launch_count<true, 0>(gt, inst, pred, N, P, vec_ok, (int)blocks, conf, (unsigned int*)work, errs, 2, s)
                                       : cs_launch_count<true, 1>(gt, inst, pred, N, P, vec_ok, (int)blocks, conf, (unsigned int*)work, errs, 2, s);
        if (!ok) return;
        hipLaunchKernelGGL(cityscapes_compact_kernel, dim3(N), dim3(1024), 0, s, (const unsigned int*)work, errs, entries, max_entries, counts);
    } else {
        if (pred_kind == 0) cs_launch_count<false, 0>(gt, nullptr, pred, N, P, vec_ok, (int)blocks, conf, nullptr, counts + 1, 3, s);
        else                cs_launch_count<false, 1>(gt, nullptr, pred, N, P, vec_ok, (int)blocks, conf, nullptr, counts + 1, 3, s);
    }
}

}  // namespace fcn8s
