// Into how many K slabs a launch cuts its dot products -- decided here and nowhere else: one named pure function per launcher that splits a
// FORWARD reduction (or a data gradient with a forward-type epilogue).  Host-only C++ (no HIP include), conv_route.h's sibling:
// tests/test_split_route_host.py builds it with a plain compiler and holds every rule to the contract below.
//
// The slab count is the summation order of every output element, and an image's forward bits must not depend on how many others share its
// batch (wino_tile_for's invariant, conv_route.h: the gradient of a batch equals the mean over its halves, a data-parallel shard computes the
// big batch's bits).  Until these rules the launchers read the TOTAL block count, which grows with N: conv5_x on a 16x16 map ran 8 slabs at
// N = 1 and 2, 5 at N = 4, one pass at N = 5.  The contract of every rule (s.N is the batch, everything else the per-image shape):
//   (1) for N >= 2 the answer does not depend on N;
//   (2) for N == 1 it may differ from the N >= 2 answer -- the one exception, as plan_N == 1 is wino_tile_for's;
//   (3) for N == 1 it is the formula the launchers had inline: batch-1 inference keeps its kernels.
// The choice for N >= 2 is ONE PASS (never split), not "split by one image's block count": a per-image count would split the score head of
// fc7 at 16 x 1024x512 (16 blocks per image, 256 in all) and conv5_x of small crops in large batches, launches that fill the chip without it
// and that the benchmark legs run unsplit.  Its cost: a batch of 2 .. 4 small images (<= 48 blocks in all) loses the split these launches
// had -- conv5_x of two 256x256 crops runs its 24 blocks of 48 K-tiles in one pass (at one image the split took such a launch from 0.046 to
// 0.030 ms, gemm_bf16.hip's note); nobody has measured the batch-2 launch itself.
// What only one launch knows -- the epilogue's form, the scratch it was given -- stays at the call site and is ANDed with the rule.
#pragma once
#include "conv_route.h"

namespace fcn8s {

constexpr int kBf16KTile = 32;          // gemm_bf16.hip's G_BK: channels of one K-tile
constexpr int kBf16RowTile = 256;       // gemm_bf16.hip's G_BM: positions of a row tile of conv_bf16_256_kernel
constexpr int kHeadSplits = 8;          // skinny.hip: the slab count of head_fwd_kernel's split form

// conv_bf16_rows_kernel, forward epilogue / unmasked data gradient of a 3x3 layer in the arithmetic of FCN8S_PREC_BF16_TRAIN.
// tile_cols x tile_rows: the form conv_bf16_rows_tile picked (64 x 256 or 128 x 128; only the 64-column form has a split).
// One image: few blocks behind many K-tiles (conv5_x: 24 blocks x 48 K-tiles) split K so that the chip fills, at least six K-tiles a slab.
inline int bf16_rows_slabs(const ConvShape& s, int tile_cols, int tile_rows)
{
    if (s.N != 1 || tile_cols != 64) return 1;
    const long long R = (long long)(s.H + 2) * (s.W + 2);
    const long long blocks = ((R + tile_rows - 1) / tile_rows) * (s.Cout / tile_cols);
    const long long nkt_all = 3LL * (s.Cin / kBf16KTile);
    if (blocks < 1 || blocks > 48 || nkt_all < 24) return 1;
    long long ks = 256 / blocks;
    if (ks > 8) ks = 8;
    if (ks > nkt_all / 6) ks = nkt_all / 6;
    return ks >= 2 ? (int)ks : 1;
}

// conv_bf16_256_kernel<256>, forward epilogue of a K != 3 layer (fc6 / fc7): one image's few output tiles behind >= 64 K-tiles, at least
// sixteen K-tiles a slab.
inline int bf16_gemm_fwd_slabs(const ConvShape& s)
{
    if (s.N != 1 || s.Cout % 256) return 1;
    const long long rt0 = ((long long)s.H * s.W + kBf16RowTile - 1) / kBf16RowTile;
    const long long tiles = rt0 * (s.Cout / 256);
    const long long nkt_all = (long long)s.K * s.K * s.Cin / kBf16KTile;
    if (tiles < 1 || tiles > 64 || nkt_all < 64) return 1;
    long long ks = 256 / tiles;
    if (ks > 8) ks = 8;
    if (ks > nkt_all / 16) ks = nkt_all / 16;
    return ks >= 2 ? (int)ks : 1;
}

// head_fwd_kernel (the fp32 1x1 score heads, Cin -> Cout = 20 or 4 classes): kHeadSplits slabs or 1.  One image of at most 64 blocks of
// 32 rows behind a reduction of whole 8 x 16 x 32 channel groups.
inline int head_fwd_splits(const ConvShape& s)
{
    if (s.N != 1) return 1;
    const long long M = (long long)s.H * s.W;
    if ((M + 31) / 32 > 64 || s.Cin % (kHeadSplits * 16 * 32) || (M * s.Cout) % 4) return 1;
    return kHeadSplits;
}

}  // namespace fcn8s
