// Calibration and error-detection counts of a softmax against its ground truth (fcn8s_op_reliability_pair; the definition is in fcn8s_hip.h):
// one pass over the N * P pixels of a batch that reads every input byte once (the softmax row 4 C B, the label id 1 B, each uncertainty map 4 B)
// and feeds four integer tables: calib [B][3], sums [4], hist [1 + J][1024][2], bad [2].  Integers only: the result does not depend on the order
// in which pixels arrive.
//
// Loads.  The batch is one flat run of N * P rows of C floats.  A block of 256 threads takes a tile of 256 consecutive pixels per trip: the
// tile's 256 C floats are brought in with lane-contiguous loads (16 bytes per lane when the base pointer is 16-byte aligned and C % 4 == 0:
// a wave's load is then 1 KiB of consecutive bytes whatever C is; 4 bytes per lane otherwise), written to an LDS image [256][S] and read back
// one row per thread.  The row stride S (in floats) is chosen so that the row reads do not conflict:
//   16-byte path  S = C if C / 4 is odd, else C + 4: rows are read with ds_read_b128, whose 16 lanes of a group then start on 16 different
//                 16-byte slots of the 256-byte bank row (l * S / 4 mod 16 is a bijection of l mod 16 for odd S / 4).  For C = 20, S = 20: the
//                 image is the tile itself and the ds_write_b128 of the fill are lane-contiguous too.  (The unpadded b32 read of a 20-float
//                 row is 4-way conflicted -- gcd(20, 32) = 4 --, which is the case the stride rule exists for.)
//   generic path  S = C if C is odd, else C + 1: rows are read with ds_read_b32 at an odd stride, 32 lanes on 32 banks.
// With C == 20 on the 16-byte path the next tile's loads (five 16-byte loads, the label byte and the scores) are issued into registers before
// the current tile is counted.  A row stride of more than 64 floats does not fit the image: such C read their rows from global memory, a
// thread per row (correct, not fast).
//
// Counting.  Block-private LDS tables, one global 64-bit atomic per non-zero entry at block end.  A trained model puts most pixels of a wave
// into one confidence bin and one uncertainty bin, so no table takes a plain per-lane atomic:
//   hist   one entry index (bin, correct | wrong) per lane and score.  rel_hist_add looks for an index that is frequent in the wave -- where one
//          is, some lane's left neighbour holds it too (one DPP move, one ballot) --, takes the first such lane as leader and lets it add the
//          pop-count of the lanes that share its index with ONE atomic; the lanes left add their 1 themselves.  Without such a pair the
//          indices are spread and nothing is aggregated.  Any order of lanes gives the same counts; an arrangement that hides a heavy index
//          from the neighbour test, or a second heavy index in the same wave, is only slower.  REL_ROUNDS leaders per call were measured at
//          0 / 1 / 2 / 4 (16 x 1024 x 512, two scores): every pixel in one entry 181 / 149 / 150 / 151 us, a concentrated but continuous
//          distribution 157 / 170 / 181 / 189 us, uniform 189 / 190 / 190 / 190 us -- each round costs a dependent scalar chain, so it is 1.
//   calib  per bin 16 slots of {count | correct << 32, sum of q_conf}, two 64-bit atomics per lane into the slot lane % 16: at most 4 lanes
//          of a wave share an address, whatever the data.  The slots are summed at block end.  (A per-bin wave reduction of the 64-bit q_conf
//          sums costs more than the two atomics at 4 lanes per address.)
//   sums, bad   per-thread 64-bit registers over the block's trips, one wave reduction at block end.
// Overflow bound of the 32-bit LDS entries: a block sees at most 2^23 tiles of 256 pixels (the launcher raises the grid when N * P asks for it), 2^31 pixels.
#include "fcn8s_internal.h"
#include <cfloat>

namespace fcn8s {

#define REL_THREADS FCN8S_REL_TILE_PIXELS
#define REL_M FCN8S_REL_SCORE_BINS
#define REL_SLOTS 16
#define REL_MAX_STRIDE 64                            // floats per row of the LDS image: 64 KB for the tile
#define REL_MAX_TRIPS (1LL << 23)
#define REL_ROUNDS 1                                 // indices a wave adds through a leader before the lanes left add their own 1

struct RelArgs {
    const float* prob; const uint8_t* gt; const uint8_t* lut;
    const float* score[3]; float scale[3];
    long long T;                                     // N * P
    int C, B, J, S;                                  // S: row stride of the LDS image in floats, 0 = rows are read from global memory
    unsigned long long *calib, *sums, *hist, *bad;
};

// row stride of the LDS image on the 16-byte path (the header comment has the rule)
__host__ __device__ constexpr int rel_vec_stride(int C) { return (C / 4) & 1 ? C : C + 4; }

// what a thread holds of a tile before it is counted: its label byte and scores, and (NV > 0) its NV 16-byte pieces of the tile's rows
template <int NV>
struct RelIn {
    float4 pv[NV > 0 ? NV : 1];
    unsigned int g;
    float s[3];
};

template <int NV>
__device__ __forceinline__ void rel_load(const RelArgs& a, long long tile, int t, RelIn<NV>& in)
{
    const long long g0 = tile * REL_THREADS;
    const long long left = a.T - g0;
    const int npx = left < REL_THREADS ? (int)left : REL_THREADS;
    if (NV > 0) {
        const float4* src = reinterpret_cast<const float4*>(a.prob + g0 * (NV * 4));
        const int nvec = npx * NV;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = t + k * REL_THREADS;
            in.pv[k] = i < nvec ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    in.g = 255u; in.s[0] = in.s[1] = in.s[2] = 0.f;
    if (t < npx) {
        in.g = a.gt[g0 + t];
#pragma unroll
        for (int j = 0; j < 3; ++j) if (j < a.J) in.s[j] = a.score[j][g0 + t];
    }
}

// bin of a value x = s * scale that is >= 0 or NaN-free by the caller's checks: min(nbins - 1, (int)x), written so that no float outside int's range is converted
__device__ __forceinline__ int rel_bin(float x, int nbins) { return x >= (float)nbins ? nbins - 1 : (x > 0.f ? (int)x : 0); }

// One row: k = argmax (lowest index on ties), conf = p_k, and the Brier sum folded in class order.  Contraction is off: the square feeds a sum.
template <bool VEC, int CT>
__device__ __forceinline__ void rel_row(const float* __restrict__ row, int C, int t, float& conf, int& best, float& brier)
{
#pragma clang fp contract(off)
    float bv = 0.f, br = 0.f; int bi = 0;
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
                const float d = v[j] - (c == t ? 1.f : 0.f);
                const float sq = d * d;
                br = br + sq;
            }
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const float v = row[c];
            if (c == 0 || v > bv) { bv = v; bi = c; }
            const float d = v - (c == t ? 1.f : 0.f);
            const float sq = d * d;
            br = br + sq;
        }
    }
    conf = bv; best = bi; brier = br;
}

// tab[idx] += 1 for every lane with `on`, aggregated over the wave (the header comment has the rule).  Called by all lanes of a wave together.
__device__ __forceinline__ void rel_hist_add(unsigned int* tab, bool on, unsigned int idx, int lane)
{
    unsigned long long rem = __ballot(on);
    // the index of the lane to the left (row_shr:1; the first lane of a row of 16 sees ~0, which is no index)
    const unsigned int left = (unsigned int)__builtin_amdgcn_update_dpp(-1, (int)idx, 0x111, 0xf, 0xf, false);
    const unsigned long long pairs = __ballot(on && left == idx);
#pragma unroll
    for (int round = 0; round < REL_ROUNDS && (pairs & rem); ++round) {
        const int leader = __ffsll((long long)(pairs & rem)) - 1;
        const unsigned int lead = (unsigned int)__builtin_amdgcn_readlane((int)idx, leader);
        const unsigned long long same = __ballot(on && idx == lead);
        if (lane == leader) atomicAdd(&tab[lead], (unsigned int)__popcll(same));
        rem &= ~same;
    }
    if ((rem >> lane) & 1ull) atomicAdd(&tab[idx], 1u);
}

__device__ __forceinline__ unsigned long long rel_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (unsigned long long)__shfl_down((long long)v, d, 64);
    return v;
}

// grid: blocks (<= tiles), block: REL_THREADS.  VEC: the 16-byte path; CT: C as a compile-time constant (next-tile loads in registers), 0 = a.C
template <bool VEC, int CT>
__global__ __launch_bounds__(REL_THREADS) void reliability_kernel(const RelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long rel_lds[];
    constexpr int NV = CT / 4;
    const int t = threadIdx.x, lane = t & 63;
    const int C = CT > 0 ? CT : a.C, S = CT > 0 ? rel_vec_stride(CT) : a.S, B = a.B, J = a.J;
    unsigned long long* cal = rel_lds;                                                         // [B][REL_SLOTS][2]
    unsigned int* hist = reinterpret_cast<unsigned int*>(cal + B * REL_SLOTS * 2);              // [1 + J][REL_M][2]
    unsigned long long* red = reinterpret_cast<unsigned long long*>(hist + (1 + J) * REL_M * 2);   // [6] (+ 2 of padding)
    uint8_t* lut = reinterpret_cast<uint8_t*>(red + 8);                                         // [256]
    float* stage = reinterpret_cast<float*>(lut + 256);                                         // [REL_THREADS][S]: every offset a multiple of 16 bytes
    for (int i = t; i < B * REL_SLOTS * 2; i += REL_THREADS) cal[i] = 0ull;
    for (int i = t; i < (1 + J) * REL_M * 2; i += REL_THREADS) hist[i] = 0u;
    if (t < 8) red[t] = 0ull;
    lut[t] = a.lut[t];                                                                          // REL_THREADS == 256 entries
    __syncthreads();

    const long long tiles = (a.T + REL_THREADS - 1) / REL_THREADS;
    unsigned long long n_all = 0, n_ok = 0, q_nll = 0, q_brier = 0, bad0 = 0, bad1 = 0;
    RelIn<NV> in;
    if ((long long)blockIdx.x < tiles) rel_load<NV>(a, blockIdx.x, t, in);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long g0 = tile * REL_THREADS;
        const long long left = a.T - g0;
        const int npx = left < REL_THREADS ? (int)left : REL_THREADS;
        if (S > 0) {
            if (NV > 0) {
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int f = (t + k * REL_THREADS) * 4, px = f / C, c = f - px * C;        // px < 256 for every k < NV
                    *reinterpret_cast<float4*>(stage + px * S + c) = in.pv[k];
                }
            } else if (VEC) {
                const float4* src = reinterpret_cast<const float4*>(a.prob + g0 * C);
                const int nvec = npx * (C / 4);
                for (int i = t; i < nvec; i += REL_THREADS) {
                    const int f = i * 4, px = f / C, c = f - px * C;
                    *reinterpret_cast<float4*>(stage + px * S + c) = src[i];
                }
            } else {
                const float* src = a.prob + g0 * C;
                const int nfl = npx * C, dq = REL_THREADS / C, dr = REL_THREADS % C;
                int px = t / C, c = t - px * C;
                for (int i = t; i < nfl; i += REL_THREADS) {
                    stage[px * S + c] = src[i];
                    px += dq; c += dr;
                    if (c >= C) { c -= C; ++px; }
                }
            }
            __syncthreads();
        }
        const unsigned int gtv = in.g;
        const float s0 = in.s[0], s1 = in.s[1], s2 = in.s[2];
        const long long next = tile + gridDim.x;
        if (next < tiles) rel_load<NV>(a, next, t, in);                                        // in flight while this tile is counted

        const unsigned int tc = t < npx ? lut[gtv & 0xFFu] : 255u;
        bool counted = false, ok = false;
        unsigned int idx[4] = {0u, 0u, 0u, 0u};
        if (tc != 255u) {
            if (tc >= (unsigned int)C) {
                ++bad0;
            } else {
                const float* row = S > 0 ? stage + t * S : a.prob + (g0 + t) * C;
                float conf, brier; int k;
                rel_row<VEC, CT>(row, C, (int)tc, conf, k, brier);
                const float pt = row[tc];
                const float sc[3] = {s0, s1, s2};
                bool fin = isfinite(conf);
#pragma unroll
                for (int j = 0; j < 3; ++j) if (j < J) fin = fin && isfinite(sc[j]);
                if (!fin) {
                    ++bad1;
                } else {
                    counted = true; ok = k == (int)tc;
                    const long long qc = (long long)rintf(conf * 16777216.f);
                    q_nll += (unsigned long long)(long long)rintf(-logf(fmaxf(pt, FLT_MIN)) * 65536.f);
                    q_brier += (unsigned long long)(long long)rintf(brier * 8388608.f);
                    ++n_all; n_ok += ok ? 1u : 0u;
                    const int b = rel_bin(conf * (float)B, B);
                    unsigned long long* slot = cal + (b * REL_SLOTS + (lane & (REL_SLOTS - 1))) * 2;
                    atomicAdd(slot, 1ull | (ok ? 1ull << 32 : 0ull));
                    atomicAdd(slot + 1, (unsigned long long)qc);
                    const unsigned int wrong = ok ? 0u : 1u;
                    const float u = 1.f - conf;
                    idx[0] = (unsigned int)(u > 0.f ? rel_bin(u * (float)REL_M, REL_M) : 0) * 2u + wrong;
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        if (j < J) idx[j + 1] = (unsigned int)(sc[j] > 0.f ? rel_bin(sc[j] * a.scale[j], REL_M) : 0) * 2u + wrong;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j <= J) rel_hist_add(hist + j * REL_M * 2, counted, idx[j], lane);
        if (S > 0) __syncthreads();                                                            // the image is free for the next tile
    }

    unsigned long long r[6] = {n_all, n_ok, q_nll, q_brier, bad0, bad1};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        r[i] = rel_wave_sum(r[i]);
        if (lane == 0 && r[i]) atomicAdd(&red[i], r[i]);
    }
    __syncthreads();
    // blocks end at about the same time: each starts its flush at another 256-entry piece of the tables, so that they do not all queue on the same addresses
    const int nh = (1 + J) * REL_M * 2, h0 = (int)(((long long)blockIdx.x * REL_THREADS) % nh);
    for (int i = t; i < nh; i += REL_THREADS) {
        const int e = i + h0 < nh ? i + h0 : i + h0 - nh;
        if (hist[e]) atomicAdd(&a.hist[e], (unsigned long long)hist[e]);
    }
    if (t < B) {
        unsigned long long n = 0, k = 0, q = 0;
#pragma unroll
        for (int s = 0; s < REL_SLOTS; ++s) {
            const unsigned long long pk = cal[(t * REL_SLOTS + s) * 2];
            n += pk & 0xFFFFFFFFull; k += pk >> 32; q += cal[(t * REL_SLOTS + s) * 2 + 1];
        }
        if (n) { atomicAdd(&a.calib[t * 3], n); atomicAdd(&a.calib[t * 3 + 2], q); }
        if (k) atomicAdd(&a.calib[t * 3 + 1], k);
    }
    if (t < 4 && red[t]) atomicAdd(&a.sums[t], red[t]);
    if (t >= 4 && t < 6 && red[t]) atomicAdd(&a.bad[t - 4], red[t]);
}

template <bool VEC, int CT>
static bool rel_launch(const RelArgs& a, int blocks, size_t lds, hipStream_t s)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&reliability_kernel<VEC, CT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "reliability_pair: %zu bytes of LDS refused (%s)", lds, hipGetErrorString(e)); return false; }
    }
    hipLaunchKernelGGL((reliability_kernel<VEC, CT>), dim3(blocks), dim3(REL_THREADS), lds, s, a);
    return true;
}

void launch_reliability_pair(const float* prob, const uint8_t* gt, const uint8_t* lut, const float* const* scores, const float* scales, int J,
                             int N, long long P, int C, int B, unsigned long long* calib, unsigned long long* sums, unsigned long long* hist,
                             unsigned long long* bad, hipStream_t s)
{
    RelArgs a = {};
    a.prob = prob; a.gt = gt; a.lut = lut;
    for (int j = 0; j < J; ++j) { a.score[j] = scores[j]; a.scale[j] = scales[j]; }
    a.T = (long long)N * P; a.C = C; a.B = B; a.J = J;
    a.calib = calib; a.sums = sums; a.hist = hist; a.bad = bad;
    bool vec = ((uintptr_t)prob & 15) == 0 && C % 4 == 0;
    int S = vec ? rel_vec_stride(C) : (C & 1 ? C : C + 1);
    if (S > REL_MAX_STRIDE) { S = 0; vec = false; }
    a.S = S;
    const long long tiles = (a.T + REL_THREADS - 1) / REL_THREADS;
    long long blocks = tiles < FCN8S_REL_MAX_BLOCKS ? tiles : FCN8S_REL_MAX_BLOCKS;
    const size_t lds = (size_t)B * REL_SLOTS * 16 + (size_t)(1 + J) * REL_M * 8 + 64 + 256 + (size_t)REL_THREADS * S * 4;
    // no more blocks than are resident at once (256 CUs, 160 KB of LDS each, at most 4 blocks per CU): a second, partly filled round of blocks
    // costs more than longer loops do, and every block ends with its own flush
    long long per_cu = (long long)(160 * 1024 / lds);
    per_cu = per_cu > 4 ? 4 : (per_cu < 1 ? 1 : per_cu);
    if (blocks > 256 * per_cu) blocks = 256 * per_cu;
    const long long need = (tiles + REL_MAX_TRIPS - 1) / REL_MAX_TRIPS;
    if (blocks < need) blocks = need;
    if (vec && C == 20) rel_launch<true, 20>(a, (int)blocks, lds, s);
    else if (vec) rel_launch<true, 0>(a, (int)blocks, lds, s);
    else rel_launch<false, 0>(a, (int)blocks, lds, s);
}

}  // namespace fcn8s
