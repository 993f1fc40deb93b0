// Boundary measures of a segmentation (fcn8s_op_boundary_pair; the definition is in fcn8s_hip.h): for a batch of N same-size images the
// trimap ring tables rings[ring - 1][gt][pred] (ring = rounded-up distance of a pixel to the nearest pixel of another ground-truth label,
// 1 .. R, R + 1 = farther) and the boundary precision / recall tables bprec / brec[ring][class] (ring = rounded-up distance of a contour
// pixel of one map to the nearest contour pixel of the same class in the other map, 0 .. R, R + 1 = unmatched).  Integers only.
//
// Shape.  A block of 512 threads owns tiles of BD_TW x BD_TH = 64 x 32 pixels (a wave per row, four rows per wave) and walks them with the
// grid's stride.  Per tile:
//   1. stage tile + halo (R for the searches, + 1 so that the halo's own contour flags can be computed) into LDS as one 32-bit word per
//      pixel: gt id | pred label id << 8 (255 = out of range, 254 = outside the image) | in B(G) << 16 | in B(P) << 17.  A row of 64
//      consecutive words is read by a wave without bank conflicts.
//      While staging, one __syncthreads_or: a staged area that is constant in both maps sends all its pixels to ring R + 1 with ONE
//      histogram update and skips everything below (the interiors of road, building and sky).
//   2. contour flags from the four neighbours, a wave per staged row.
//   3. in the same pass as the flags, per staged row a bit mask of the horizontal label changes (G[x] != G[x + 1], both inside the image)
//      by two wave ballots, and from it h = the distance of a pixel to the nearest other label in its own row (one shift, one count-trailing
//      and one count-leading zeros) into the top byte of its word.
//   4. search 1 (rings): d2(p) = min over dy of dy^2 + (G[p + dy] != G[p] ? 0 : h(p + dy)^2): 2R + 1 taps of one LDS word each instead of
//      (2R + 1)^2, four row pairs in flight at a time, ended once dy^2 reaches the best distance so far.
//   5. search 3 (bprec / brec): contour pixels only, a tile row (one wave) at a time and one class at a time: the staged rows around it
//      become bit masks of "contour pixel of the other map with this class" by ballots, and every lane of the class reads its nearest set
//      bit off them (bd_match_row).  A per-lane walk over the disk (rows by |dy|, columns by |dx|, cut off by the best distance) was
//      measured first: a contour pixel whose class is absent nearby walks all (2R + 1)^2 offsets while its wave waits, which on
//      Cityscapes-like maps (4 x 2048x1024) cost 1348 us at R = 8 and 6676 us at R = 16 where this search, before anything else was
//      tuned, took 523 and 1445.  Pure noise prefers the per-lane walk (407 us against 2315 at R = 3: dozens of classes per row here, and
//      there a match after a few taps); real label maps are the workload.
//   6. counts go to block-private LDS histograms.  The ring keys of a wave (one image row of 64 pixels, a handful of distinct keys on a
//      real label map) are folded with ballots first: up to BD_FOLD distinct keys cost one LDS atomic each, what is left (noise) one per lane.
// At the end of the block one 64-bit global atomic per non-zero bin.
//   Bounds.  LDS bins are 32 bits: the launcher gives a block at most 2^20 tiles = 2^31 pixels.  Every staged read is at most R rows /
// columns away from a tile pixel, which lies BD_HALO = R + 1 inside the staged area.
#include "fcn8s_internal.h"

namespace fcn8s {

#define BD_THREADS 512
#define BD_TW 64
#define BD_TH 32
#define BD_IDS 34
#define BD_CONF (BD_IDS * BD_IDS)
#define BD_FOLD 4
#define BD_OUTSIDE 254u
#define BD_BAD 255u
#define BD_NOKEY 0xFFFFFFFFu
#define BD_MAX_BLOCKS 1024                           // measured: 512 .. 4096 within 20 % of each other (more gain at R = 3, lose at R = 16), 256 is 1.7 x slower at R = 3
#define BD_MAX_TILES_PER_BLOCK (1LL << 20)
#define BD_STAGE_ROWS 9                              // ceil((BD_TH + 2 * 17) / 8 waves)

__device__ __forceinline__ unsigned int bd_train_to_label(unsigned int t)       // labels.py trainId -> id, t < 20 (as in cityscapes.hip)
{
    const unsigned long long w = t < 8 ? 0x13110D0C0B080700ull : (t < 16 ? 0x1B1A191817161514ull : 0x0000000021201F1Cull);
    return (unsigned int)(w >> ((t & 7) * 8)) & 0xFFu;
}

__device__ __forceinline__ int bd_ring(int d2, int R)                           // smallest k >= 0 with k^2 >= d2; R + 1 beyond R
{
    if (d2 > R * R) return R + 1;
    int k = 0;
    while (k * k < d2) ++k;
    return k;
}

// the staged word of pixel q: gt id | pred label id << 8, an id out of range as BD_BAD
template <int KIND>
__device__ __forceinline__ unsigned int bd_load(const uint8_t* __restrict__ gt, const void* __restrict__ pred, long long q)
{
    unsigned int g = gt[q], p;
    if (KIND == 0) {
        const unsigned long long v = (unsigned long long)reinterpret_cast<const long long*>(pred)[q];
        p = v < 20ull ? bd_train_to_label((unsigned int)v) : BD_BAD;
    } else {
        p = reinterpret_cast<const uint8_t*>(pred)[q];
    }
    if (g >= BD_IDS) g = BD_BAD;
    if (p >= BD_IDS) p = BD_BAD;
    return g | p << 8;
}

// Search 3 for one tile row (a wave; lane = column): every lane with cls != BD_NOKEY looks for the nearest staged pixel whose word w has
// (w & mask) == (flag | cls << shift) -- a contour pixel of the other map with the lane's class -- and counts the ring of its squared
// distance in h[ring][cls].  The wave works through the distinct classes of its lanes one at a time (a handful on a real label map): for
// the class in turn it walks the staged rows sy, sy +- 1, ... and turns each into a bit mask of the matching columns with two ballots; a
// lane reads the nearest set bit around its own column off that mask.  The walk ends as soon as no lane of the class can still improve
// (dy^2 >= its best), so matched contours cost a few rows and only a class that is absent nearby costs all 2R + 1.  Uniform over the wave.
__device__ __forceinline__ void bd_match_row(const unsigned int* __restrict__ st, int SW, int sy, int lane, int R, unsigned int cls,
                                             unsigned int mask, unsigned int flag, int shift, unsigned int* __restrict__ h)
{
    const int sx = lane + R + 1, s0 = sx - R;                                    // the window of 2R + 1 columns starts at s0, 1 <= s0 <= 64
    const unsigned int lowR = (1u << R) - 1u, lowR1 = (2u << R) - 1u;
    for (;;) {
        const unsigned long long act = __ballot(cls != BD_NOKEY);
        if (!act) break;
        const unsigned int c = (unsigned int)__shfl((int)cls, __ffsll((long long)act) - 1, 64);
        const bool mine = cls == c;
        const unsigned int want = flag | c << shift;
        int best = R * R + 1;
        for (int d = 0; d <= R; ++d) {
            const int dd = d * d;
            if (!__ballot(mine && best > dd)) break;
            const unsigned int* ra = st + (sy + d) * SW;
            const unsigned int* rb = st + (sy - d) * SW;                          // d = 0: the same row twice
            const int l2 = lane + 64 < SW ? lane + 64 : lane;
            const unsigned int a0 = ra[lane], a1 = ra[l2], b0 = rb[lane], b1 = rb[l2];
            const unsigned long long lo[2] = {__ballot((a0 & mask) == want), __ballot((b0 & mask) == want)};
            const unsigned long long hi[2] = {__ballot(lane + 64 < SW && (a1 & mask) == want), __ballot(lane + 64 < SW && (b1 & mask) == want)};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!(lo[k] | hi[k])) continue;
                const unsigned long long win = s0 < 64 ? (lo[k] >> s0) | (hi[k] << (64 - s0)) : hi[k] >> (s0 - 64);
                const unsigned int left = (unsigned int)win & lowR, right = (unsigned int)(win >> R) & lowR1;      // right: bit 0 = the lane's own column
                int e = R + 1;
                if (right) e = __ffs(right) - 1;
                if (left) { const int el = R - (31 - __clz(left)); if (el < e) e = el; }
                if (e <= R) { const int d2 = dd + e * e; if (d2 < best) best = d2; }
            }
        }
        if (mine) { atomicAdd(&h[bd_ring(best, R) * BD_IDS + c], 1u); cls = BD_NOKEY; }
    }
}

template <int KIND>
__global__ __launch_bounds__(BD_THREADS) void boundary_kernel(const uint8_t* __restrict__ gt_all, const void* __restrict__ pred_all, int N, int H, int W, int R,
                                                              int tiles_x, int tiles_y, unsigned long long* __restrict__ rings,
                                                              unsigned long long* __restrict__ bprec, unsigned long long* __restrict__ brec,
                                                              unsigned long long* __restrict__ bad)
{
    extern __shared__ unsigned long long bd_lds[];
    const int HALO = R + 1, SW = BD_TW + 2 * HALO, SH = BD_TH + 2 * HALO;
    const int nring = (R + 1) * BD_CONF, nb = (R + 2) * BD_IDS;
    unsigned int* st = reinterpret_cast<unsigned int*>(bd_lds);                  // [SH][SW] staged words
    unsigned int* hist = st + SH * SW;                                           // [R + 1][34][34]
    unsigned int* hp = hist + nring;                                             // [R + 2][34]
    unsigned int* hr = hp + nb;                                                  // [R + 2][34]
    unsigned int* hbad = hr + nb;                                                // [1]
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int i = t; i < nring + 2 * nb + 1; i += BD_THREADS) hist[i] = 0u;
    __syncthreads();

    const long long P = (long long)H * W;
    const long long ntiles = (long long)N * tiles_y * tiles_x;
    unsigned int nbad = 0;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int n = (int)(tile / ((long long)tiles_y * tiles_x));
        const int rem = (int)(tile - (long long)n * tiles_y * tiles_x);
        const int y0 = (rem / tiles_x) * BD_TH, x0 = (rem % tiles_x) * BD_TW;
        const uint8_t* gt = gt_all + (long long)n * P;
        const void* pred = KIND == 0 ? (const void*)(reinterpret_cast<const long long*>(pred_all) + (long long)n * P)
                                     : (const void*)(reinterpret_cast<const uint8_t*>(pred_all) + (long long)n * P);

        // 1. stage, a wave per staged row; `differs`: some staged pixel inside the image is not the tile's first pixel
        const unsigned int ref = bd_load<KIND>(gt, pred, (long long)y0 * W + x0);
        int differs = 0;
        {
            // SH <= 66 rows over 8 waves: at most BD_STAGE_ROWS = 9 per wave, unrolled so that all of a wave's loads are issued before the first
            // is used.  Measured against the plain loop over the rows on constant maps (staging only): 67 / 80 / 175 us against 61 / 76 / 168
            // for 4 x 2048x1024 at R = 3 / 8 / 16 -- no gain: the load latency is not what staging waits for (profiles/trimap_eval_probes.txt)
            unsigned int wr[BD_STAGE_ROWS][2];
#pragma unroll
            for (int k = 0; k < BD_STAGE_ROWS; ++k) {
                const int sy = wv + k * (BD_THREADS / 64), y = y0 - HALO + sy;
                const bool rowin = sy < SH && y >= 0 && y < H;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int sx = half * 64 + lane, x = x0 - HALO + sx;
                    wr[k][half] = BD_OUTSIDE | BD_OUTSIDE << 8;
                    if (rowin && sx < SW && x >= 0 && x < W) wr[k][half] = bd_load<KIND>(gt, pred, (long long)y * W + x);
                }
            }
#pragma unroll
            for (int k = 0; k < BD_STAGE_ROWS; ++k) {
                const int sy = wv + k * (BD_THREADS / 64);
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int sx = half * 64 + lane;
                    if (sy < SH && sx < SW) {
                        st[sy * SW + sx] = wr[k][half];
                        differs |= wr[k][half] != ref && wr[k][half] != (BD_OUTSIDE | BD_OUTSIDE << 8);
                    }
                }
            }
        }
        if (!__syncthreads_or(differs)) {
            // a constant staged area: every tile pixel inside the image in ring R + 1, no contour (nothing reads st: no second barrier)
            if (t == 0) {
                const unsigned int g = ref & 0xFFu, p = ref >> 8;
                const unsigned int cnt = (unsigned int)((H - y0 < BD_TH ? H - y0 : BD_TH) * (W - x0 < BD_TW ? W - x0 : BD_TW));
                if (g == BD_BAD || p == BD_BAD) nbad += cnt;
                else atomicAdd(&hist[R * BD_CONF + g * BD_IDS + p], cnt);
            }
            continue;
        }

        // 2. a wave per staged row (the outermost ring is never searched): contour flags into bits 16 / 17 of the words (other waves read
        // only the low 16 bits meanwhile), the row's label-change mask (bit x = G[x] != G[x + 1], both inside the image) by two ballots,
        // and from it, for the tile's columns, h = the distance to the nearest other label in this row (R + 1: none within R) into the
        // word's top byte
        const unsigned int lowR = (1u << R) - 1u;
        for (int sy = 1 + wv; sy < SH - 1; sy += BD_THREADS / 64) {
            unsigned int* row = st + sy * SW;
            unsigned int wq[2] = {0u, 0u}, fq[2] = {0u, 0u};
            bool eq[2] = {false, false};
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int sx = half * 64 + lane;
                if (sx + 1 < SW) {
                    const unsigned int w = row[sx] & 0xFFFFu, rgt = row[sx + 1] & 0xFFFFu;
                    wq[half] = w;
                    eq[half] = (w & 0xFFu) != (rgt & 0xFFu) && (w & 0xFFu) != BD_OUTSIDE && (rgt & 0xFFu) != BD_OUTSIDE;
                    if (sx > 0 && (w & 0xFFu) != BD_OUTSIDE) {
                        const unsigned int nbr[4] = {row[sx - SW] & 0xFFFFu, row[sx + SW] & 0xFFFFu, row[sx - 1] & 0xFFFFu, rgt};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if ((nbr[k] & 0xFFu) == BD_OUTSIDE) continue;
                            if ((nbr[k] & 0xFFu) != (w & 0xFFu)) fq[half] |= 0x10000u;
                            if ((nbr[k] >> 8) != (w >> 8)) fq[half] |= 0x20000u;
                        }
                    }
                }
            }
            const unsigned long long lo = __ballot(eq[0]), hi = __ballot(eq[1]);
#pragma unroll
            for (int half = 0; half < 2; ++half)
                if (fq[half]) row[half * 64 + lane] = wq[half] | fq[half];
            const int s0 = lane + 1;                                             // column HALO + lane: its window of changes starts at HALO + lane - R
            const unsigned long long win = s0 < 64 ? (lo >> s0) | (hi << (64 - s0)) : hi;
            const unsigned int left = (unsigned int)win & lowR, right = (unsigned int)(win >> R) & lowR;
            int h = R + 1;
            if (right) h = __ffs(right);                                         // change between x + j and x + j + 1: distance j + 1
            if (left) { const int hl = R - (31 - __clz(left)); if (hl < h) h = hl; }
            reinterpret_cast<unsigned char*>(row + HALO + lane)[3] = (unsigned char)h;                      // after the word stores of this wave
        }
        __syncthreads();

        // 3. - 5. four rows per wave, a lane per column
        for (int r = wv; r < BD_TH; r += BD_THREADS / 64) {
            const int sy = HALO + r, sx = HALO + lane;
            const unsigned int w = st[sy * SW + sx], g = w & 0xFFu, p = (w >> 8) & 0xFFu;
            unsigned int key = BD_NOKEY, cp = BD_NOKEY, cg = BD_NOKEY;
            if (g != BD_OUTSIDE) {
                if (g == BD_BAD || p == BD_BAD) {
                    ++nbad;
                } else {
                    // search 1: d2 = min over dy of dy^2 + (another label in that row of this column ? 0 : h^2)
                    const int big = R * R + 1, h0 = (int)(w >> 24);
                    int best = h0 <= R ? h0 * h0 : big;
                    for (int d0 = 1; d0 <= R && d0 * d0 < best; d0 += 4) {        // four row pairs at a time: eight LDS reads in flight
                        unsigned int wa[4], wb[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int d = d0 + j <= R ? d0 + j : R;               // beyond R: row R once more (harmless)
                            wa[j] = st[(sy + d) * SW + sx]; wb[j] = st[(sy - d) * SW + sx];
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int d = d0 + j <= R ? d0 + j : R, dd = d * d;
                            const int ha = (int)(wa[j] >> 24), hb = (int)(wb[j] >> 24);
                            int ca = (wa[j] & 0xFFu) != g ? dd : (ha <= R ? dd + ha * ha : big);
                            int cb = (wb[j] & 0xFFu) != g ? dd : (hb <= R ? dd + hb * hb : big);
                            if ((wa[j] & 0xFFu) == BD_OUTSIDE) ca = big;
                            if ((wb[j] & 0xFFu) == BD_OUTSIDE) cb = big;
                            best = min(best, min(ca, cb));
                        }
                    }
                    key = (unsigned int)((bd_ring(best, R) - 1) * BD_CONF) + g * BD_IDS + p;
                    if (w & 0x20000u) cp = p;                                    // on a contour of P: look for a contour pixel of G with label p
                    if (w & 0x10000u) cg = g;                                    // and the other way round
                }
            }
            bd_match_row(st, SW, sy, lane, R, cp, 0x100FFu, 0x10000u, 0, hp);
            bd_match_row(st, SW, sy, lane, R, cg, 0x2FF00u, 0x20000u, 8, hr);
            // fold the wave's equal keys (the loop is uniform over the wave)
            for (int round = 0; round < BD_FOLD; ++round) {
                const unsigned long long act = __ballot(key != BD_NOKEY);
                if (!act) break;
                const int leader = __ffsll((long long)act) - 1;
                const unsigned int k0 = (unsigned int)__shfl((int)key, leader, 64);
                const unsigned long long same = __ballot(key == k0);
                if (lane == leader) atomicAdd(&hist[k0], (unsigned int)__popcll(same));
                if (key == k0) key = BD_NOKEY;
            }
            if (key != BD_NOKEY) atomicAdd(&hist[key], 1u);
        }
        __syncthreads();                                                         // st is restaged by the next tile
    }
    if (nbad) atomicAdd(hbad, nbad);
    __syncthreads();

    for (int i = t; i < nring; i += BD_THREADS)
        if (hist[i]) atomicAdd(&rings[i], (unsigned long long)hist[i]);
    for (int i = t; i < nb; i += BD_THREADS) {
        if (hp[i]) atomicAdd(&bprec[i], (unsigned long long)hp[i]);
        if (hr[i]) atomicAdd(&brec[i], (unsigned long long)hr[i]);
    }
    if (t == 0 && *hbad) atomicAdd(bad, (unsigned long long)*hbad);
}

template <int KIND>
static void bd_launch(const uint8_t* gt, const void* pred, int N, int H, int W, int R, unsigned long long* rings, unsigned long long* bprec,
                      unsigned long long* brec, unsigned long long* bad, hipStream_t s)
{
    const int HALO = R + 1, SW = BD_TW + 2 * HALO, SH = BD_TH + 2 * HALO;
    const size_t lds = (size_t)SH * SW * 4 + ((size_t)(R + 1) * BD_CONF + 2 * (size_t)(R + 2) * BD_IDS + 1) * 4;    // 109.4 KB at R = 16
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&boundary_kernel<KIND>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { defer_error(FCN8S_ERR_HIP, "boundary_pair: %zu bytes of LDS refused (%s)", lds, hipGetErrorString(e)); return; }
    }
    const int tiles_x = (W + BD_TW - 1) / BD_TW, tiles_y = (H + BD_TH - 1) / BD_TH;
    const long long ntiles = (long long)N * tiles_y * tiles_x;
    long long blocks = ntiles < BD_MAX_BLOCKS ? ntiles : BD_MAX_BLOCKS;
    const long long need = (ntiles + BD_MAX_TILES_PER_BLOCK - 1) / BD_MAX_TILES_PER_BLOCK;      // 32-bit LDS bins: at most 2^31 pixels per block
    if (blocks < need) blocks = need;
    hipLaunchKernelGGL((boundary_kernel<KIND>), dim3((unsigned int)blocks), dim3(BD_THREADS), lds, s, gt, pred, N, H, W, R, tiles_x, tiles_y, rings, bprec, brec, bad);
}

void launch_boundary_pair(const uint8_t* gt, const void* pred, int pred_kind, int N, int H, int W, int R, unsigned long long* rings,
                          unsigned long long* bprec, unsigned long long* brec, unsigned long long* bad, hipStream_t s)
{
    if (pred_kind == 0) bd_launch<0>(gt, pred, N, H, W, R, rings, bprec, brec, bad, s);
    else                bd_launch<1>(gt, pred, N, H, W, R, rings, bprec, brec, bad, s);
}

}  // namespace fcn8s
