// Which kernels a convolution layer of fcn8s_model runs through -- direct, Winograd F(2x2) / F(4x4) / F(6x6), the adjoint data gradient, the fused
// transforms, the pool routed inside a transform, the dM hand-off -- decided here and nowhere else: one named pure function per decision.
// Host-only C++ (no HIP include): tests/test_conv_route_host.py builds it with a plain compiler and checks the implications the launch sequences
// of model.hip rely on.  pass_state.h records what a pass DID; this header says what a pass WILL do.
//
// A rule sees the options (RouteOpts) and the shape of the FORWARD convolution (ConvShape: Cin -> Cout channels on an H x W map), or two adjacent
// layers where the decision spans two.  What only one launch knows -- training or not, a per-launch option, the precision branch, an epilogue that
// asks for alpha != 1, real_cin or dropout -- stays at the call site and is ANDed with the rule.
#pragma once
#include <algorithm>

namespace fcn8s {

// the option fields the rules read (route_opts() in model.hip fills it from an fcn8s_model).  Every one of them drops the workspace when it
// changes (fcn8s_set_option), and plan_N is set by the plan itself: a fact derived from them holds for as long as the arena it was planned for.
struct RouteOpts {
    int wino_min_cin = 64;           // 3x3 layers with Cin >= this use Winograd; 0 = never
    int wino_tile = 6;               // largest 3x3 output tile
    int wino_tile_hires = 0, wino_hires_pixels = 0;      // != 0: maps of at least wino_hires_pixels pixels use at most wino_tile_hires
    int wino_force_tile = 0;         // != 0: every eligible 3x3 layer uses exactly this tile (op-level parity entry point)
    int wino_fc6 = 1;                // fc6 7x7 as a 2x2 grid of 4x4 sub-filters in the Winograd domain
    int plan_N = 0;                  // the batch size the workspace was planned for
    bool scratch = false;            // the shared V / M scratch (wino_v, wino_m) exists
};
struct ConvShape { int N, H, W, Cin, Cout, K; };
inline ConvShape transposed(ConvShape s) { std::swap(s.Cin, s.Cout); return s; }      // the data gradient's convolution: dY (Cout channels) -> dX (Cin)

// Output tile of the Winograd path for a K x K SAME conv on an H x W map (0 = none).  K = 7 (fc6): 4 (sub-filter decomposition).
// K = 3: F(6x6) [64 positions per 36 outputs, partial edge tiles] or F(4x4) [36 per 16, needs H, W % 4 == 0], whichever multiplies
// less on this map (small maps lose more to F(6x6)'s partial tiles than they gain); F(2x2) as the fallback.
inline int wino_tile_for(const RouteOpts& o, int H, int W, int K = 3)
{
    if (H % 2 || W % 2) return 0;
    if (o.wino_force_tile && K == 3) return (o.wino_force_tile == 6 || (H % o.wino_force_tile == 0 && W % o.wino_force_tile == 0)) ? o.wino_force_tile : 0;
    int tmax = o.wino_tile;
    if (K == 3 && o.wino_tile_hires && o.wino_hires_pixels > 0 && (long long)H * W >= o.wino_hires_pixels && o.wino_tile_hires < tmax) tmax = o.wino_tile_hires;
    const bool t4 = tmax >= 4 && H % 4 == 0 && W % 4 == 0;
    if (K == 7) return (o.wino_tile >= 4 && H % 4 == 0 && W % 4 == 0) ? 4 : 0;
    if (tmax == 6) {
        // multiplies per channel pair = positions x GEMM rows.  For a single image the rows are rounded up to the 64-row GEMM tile: a 32x64
        // map has 66 F(6x6) tiles -- two row tiles, the second one nearly empty -- but exactly 128 F(4x4) tiles.  Batches of two or more
        // images are NOT treated this way: the arithmetic applied to an image must not depend on how many others share its batch (the
        // gradient of a batch equals the mean over its halves, data-parallel shards equal the big batch).
        auto rows = [&](long long tiles) { return o.plan_N == 1 ? (tiles + 63) / 64 * 64 : tiles; };
        const long long c6 = 64LL * rows((long long)((H + 5) / 6) * ((W + 5) / 6)), c4 = t4 ? 36LL * rows((long long)(H / 4) * (W / 4)) : 16LL * rows((long long)(H / 2) * (W / 2));
        if (c6 < c4) return 6;
    }
    return t4 ? 4 : 2;
}

// ---- one convolution ------------------------------------------------------------------------------------------------------------------------
// The shape half of "this K x K conv Cin -> Cout runs through Winograd": the tile (0 = direct).  3x3 from wino_min_cin input channels up, fc6's
// 7x7 with option winograd_fc6; the position GEMMs want whole 16-channel K steps and 64-column tiles.
inline int wino_shape_tile(const RouteOpts& o, const ConvShape& s)
{
    if (s.Cin % 16 || s.Cout % 64) return 0;
    if (s.K == 3) return (o.wino_min_cin > 0 && s.Cin >= o.wino_min_cin) ? wino_tile_for(o, s.H, s.W, 3) : 0;
    if (s.K == 7) return (o.wino_fc6 && wino_tile_for(o, s.H, s.W, 7) == 4) ? 4 : 0;
    return 0;
}
// Forward Winograd tile, 0 = direct: the shape rule, in a workspace that has the scratch.
inline int fwd_tile(const RouteOpts& o, const ConvShape& s) { return o.scratch ? wino_shape_tile(o, s) : 0; }
// The forward pass keeps the layer's V for its weight gradient (slot "wv:<layer>", 3x3 layers; fc6's slot is sized by fc6_scratch_floats).
// A plan-time question -- the scratch is sized by the same plan, scratch_channels() -- so it asks the shape rule alone.
inline bool keeps_v(const RouteOpts& o, const ConvShape& s) { return s.K == 3 && wino_shape_tile(o, s) != 0; }
// fc6's slot "wv:fc6" is planned only in a workspace whose 3x3 layers may keep theirs: with winograd_min_cin = 0 fc6 still runs F(4x4,4x4) forward
// (option winograd_fc6) but its weight gradient takes the direct taps.  Kept as found.
inline bool fc6_keeps_v(const RouteOpts& o) { return o.wino_min_cin > 0; }
// Data gradient through Winograd: the forward algorithm on the flipped + transposed kernel, i.e. the same rule for the transposed conv.  ANY tile:
inline int dgrad_tile(const RouteOpts& o, const ConvShape& s) { return fwd_tile(o, transposed(s)); }
// ... but its input transform is written by the weight gradient's dY transform (one read of dZ) only by the F(4x4) / F(6x6) kernels: tile >= 4
// (wino_input_dout_kernel has no F(2x2) form; such a layer's data gradient still runs through Winograd, with a transform of its own).
inline bool dgrad_input_fused(const RouteOpts& o, const ConvShape& s) { return s.K == 3 && dgrad_tile(o, s) >= 4; }
// Adjoint data gradient, dV = dM U^T from the weight gradient's dM and the forward filter bank: F(6x6) and both widths whole 64-channel tiles.
// The weight gradient (which then writes dM alone, no V) and the data gradient (which takes it) both ask here.
inline bool adjoint_dgrad(const RouteOpts& o, const ConvShape& s) { return s.K == 3 && dgrad_tile(o, s) == 6 && s.Cin % 64 == 0 && s.Cout % 64 == 0; }
// The adjoint data gradients read the forward filter bank of the same step as a transposed B operand (gemm_glds_nt_kernel).  That kernel
// only exists in the LDS-DMA form: K % 16 == 0 and whole N tiles of the width launch_igemm picks (64 for N = 64, else 128).  Other widths
// (e.g. 192) get a second, transposed bank instead (3x3 layers) or the forward-type data gradient (fc6).
inline bool bt_gemm_ok(int K, int N) { return K % 16 == 0 && (N == 64 || N % 128 == 0); }
// fc6's adjoint data gradient asks less than dgrad_tile: it finds dM and this step's forward bank (the forward pass and the weight gradient ran
// F(4x4,4x4)) and multiplies on the transposed-bank GEMM, whose width rule is bt_gemm_ok -- not the 64-column tiles of a forward-type launch.
inline bool fc6_wino_map(const RouteOpts& o, int H, int W) { return o.wino_fc6 && o.scratch && wino_tile_for(o, H, W, 7) == 4; }
// Channels the shared scratch is sized for on this layer's map, 0 = none.  Looser than wino_shape_tile on purpose: either width counts and nothing
// is asked of divisibility, because the data gradient swaps the two roles and an arena that is too large is harmless, one too small is not.
inline int scratch_channels(const RouteOpts& o, const ConvShape& s)
{
    return (o.wino_min_cin > 0 && std::max(s.Cin, s.Cout) >= o.wino_min_cin && wino_tile_for(o, s.H, s.W, s.K)) ? std::max(s.Cin, s.Cout) : 0;
}

// ---- two adjacent layers of a block (next: the conv that reads l's output on the same map) ---------------------------------------------------
// ReLU bit record of l's output ("rb:<layer>"), read by next's data gradient instead of the tensor: who writes it.
enum class RbWriter { none, self, consumer };
// self: l's own Winograd output transform.  consumer: conv1_1 is never a Winograd layer (3 input channels); its record comes out of conv1_2's
// input transform.  Only conv1_1 gets that: another direct layer in front of a Winograd one (winograd_min_cin = 128: conv3_1) has no record and
// its consumer's data gradient masks with the tensor.
inline RbWriter relu_record_writer(const RouteOpts& o, const ConvShape& l, const ConvShape& next, bool l_is_conv1_1)
{
    if (l_is_conv1_1 && l.Cout % 64 == 0 && keeps_v(o, next)) return RbWriter::consumer;
    return keeps_v(o, l) ? RbWriter::self : RbWriter::none;
}
// l's output transform writes next's V directly (l's activation is never written): both run F(6x6,3x3), hence on one tile grid.
inline bool out_in_fused(const RouteOpts& o, const ConvShape& l, const ConvShape& next) { return l.K == 3 && next.K == 3 && fwd_tile(o, l) == 6 && fwd_tile(o, next) == 6; }
// conv1_1 is evaluated inside conv1_2's F(6x6,3x3) input transform (wino_input_conv1_kernel: 64 output channels, conv1_2 the block's last conv)
inline bool conv1_in_next_transform(const RouteOpts& o, const ConvShape& conv1_1, const ConvShape& next) { return conv1_1.Cout == 64 && fwd_tile(o, next) == 6; }
// next's adjoint data gradient writes l's dM instead of its dZ.  l's weight gradient must then take the prefilled adjoint branch (it keeps V,
// adjoint_dgrad(l)); the promise is only ever made inside next's adjoint data gradient (adjoint_dgrad(next)).
inline bool dm_from_next(const RouteOpts& o, const ConvShape& l)
{
    return o.scratch && keeps_v(o, l) && wino_tile_for(o, l.H, l.W, 3) == 6 && l.Cin % 64 == 0 && l.Cout % 64 == 0;
}
// d(pool) is routed through the argmax bytes inside the transform shared by the gradients of the block's last conv (neither its dZ nor its
// full-resolution output is read again): that conv keeps V and its data gradient's input transform is fused -- which needs a conv in front of it
// in the block (has_prev: Cin == Cout == the block's width).
inline bool pool_in_transform(const RouteOpts& o, const ConvShape& last, bool has_prev)
{
    return o.wino_min_cin > 0 && last.Cout >= o.wino_min_cin && o.scratch && wino_tile_for(o, last.H, last.W, 3) >= 4 && last.Cout % 64 == 0 && has_prev && keeps_v(o, last);
}
// The block's last conv runs its 64 position GEMMs, the output transform and the pool in ONE kernel (wino_gemm_out64_kernel: a block owns all 64
// positions of 16 tiles, M is never written): F(6x6,3x3), 64 -> 64 channels, and the pool its output's only reader -- conv1_2.  It reads the
// layer's shape and never N: which tiles share a block changes no tile's arithmetic, and an image's result must not depend on its batch
// (wino_tile_for's invariant; the batch enters only where it enters the tile itself, plan_N == 1 on small maps, and with the tile the whole
// algorithm changes anyway).  The layer's filter bank is then kept twice: the standard one and the kernel's MFMA-ordered copy behind it.
// Only conv1_2 gets that (last_is_conv1_2: the last conv of block 1): it is the layer the kernel was built and measured for -- the full-resolution
// map, where M's round trip is 7.7 GB per launch.  A 64-wide last conv of a deeper block (narrow models: a few tiles per image) keeps the two kernels
// and, with them, the arithmetic the suite's tightest bounds on such models were measured with.
// (The op-level entry points fcn8s_op_conv3x3_winograd_fwd_bwd / _pool have one layer and no table: they set the caller's flag from the op context
// "op_gemm_out_fused64", default 0, and conv_winograd's own conditions decide as for a model.)
inline bool gemm_out_fused64(const RouteOpts& o, const ConvShape& last, bool has_prev, bool last_is_conv1_2)
{
    return last_is_conv1_2 && last.K == 3 && last.Cin == 64 && last.Cout == 64 && fwd_tile(o, last) == 6 && pool_in_transform(o, last, has_prev);
}

// ---- FCN8S_PREC_BF16_TRAIN: which fp32 tensor a pass keeps, which it skips -------------------------------------------------------------------------
// The mode runs every convolution but conv1_1 on the bf16 kernels (gemm_bf16.hip), forward and backward, and hands an activation or a gradient on as
// the READER's padded bf16 copy.  The forward pass may skip an fp32 tensor only if every later reader provably takes the bf16 form: the rules below
// are both sides of that promise -- what forward() skips, and what backward_blocks / conv_wgrad / conv_dgrad will ask for
// (tests/test_bf16_route_host.py checks the implications between them).
// PRECONDITION of the mode, stated once: every one of the seven widths is a multiple of 64 (fcn8s_set_precision refuses the mode otherwise) and every
// kernel size is odd (fcn8s_create).  conv1_1 (3 input channels, padded to 4) is therefore the ONLY layer with Cin % 64 != 0, and a block's last conv
// always has a conv of the same width in front of it: Cin == Cout.
// The per-launch options the rules read (bf16_opts() in model.hip fills it, per pass).  None of them drops the arena, so no fact derived from them
// is stored in the layer table: the call sites evaluate the rules in every pass.
struct Bf16Opts {
    bool acts = true;                // option bf16_acts: a conv -> conv activation is kept only as the consumer's padded bf16 copy
    bool fuse_pool = true;           // option bf16_fuse_pool: the pools keep routing bytes and read / write the bf16 copies
    bool conv1_tiled = true;         // option conv1_tiled: conv1_1 on the spatial-tile kernel (the only one that writes a bf16 copy)
    bool copies = true;              // the pass makes per-layer copies at all: training, or option bf16_infer_copies
};
// The one width / kernel-size test: the bf16 convolution and weight-gradient kernels take the layer (gemm_bf16.hip's own checks stay the kernels'
// contract).  forward(), backward_blocks, conv_wgrad ask it of the forward shape, conv_dgrad of the transposed one.
inline bool bf16_kernels_take(const ConvShape& s) { return s.Cin % 64 == 0 && s.Cout % 64 == 0 && s.K % 2 == 1; }
// pool3 / pool4 also feed the fp32 skip heads (1-based block): their blocks keep the fp32 tensors.  forward()'s conv, pool and fp8 stages ask.
inline bool pool_feeds_skip(int block) { return block == 3 || block == 4; }
// The 32-bit per-lane byte offsets of the weight-gradient kernels span TWO 32-channel planes of a padded copy (launch_wgrad_bf16's limit, asked by
// forward() before anything is launched): a plane of plane_elems bf16 elements must stay below 4 GiB.  Kept as found, including that it is vacuous
// in a library built with A_PLANES = 0 (plane stride 0) -- a known finding, not this rule's to fix.
inline bool bf16_plane_fits(long long plane_elems) { return (double)plane_elems * 2.0 + 65536.0 < 4294967296.0; }

// -- forward: a convolution's output --
// conv1_1 writes conv1_2's padded bf16 input copy and no fp32 tensor (the 64-wide tile kernel on a map of whole 8 x 16 tiles; the caller has
// checked that conv1_1 takes the gather kernel at all).  conv1_2's gradients are then the tensor's only readers, in its bf16 form.
inline bool conv1_writes_bf16_only(const Bf16Opts& o, const ConvShape& conv1_1, const ConvShape& next)
{
    return o.copies && o.acts && o.conv1_tiled && conv1_1.H % 8 == 0 && conv1_1.W % 16 == 0 && conv1_1.Cout % 64 == 0 && bf16_kernels_take(next);
}
// a conv's epilogue writes the in-block consumer's padded bf16 input copy (has_next: there is such a consumer)
inline bool out_bf16_copy(const Bf16Opts& o, bool has_next) { return o.copies && o.acts && has_next; }
// ... and that copy is the output's only form: the fp32 tensor is not written.  Its readers are the consumer's weight gradient (its input) and data
// gradient (the ReLU mask: the sign of the copy) -- both must fit the bf16 kernels, a fallback would look for the fp32 tensor.
inline bool out_bf16_only(const Bf16Opts& o, const ConvShape& l, const ConvShape& consumer)
{
    return out_bf16_copy(o, true) && bf16_kernels_take(l) && bf16_kernels_take(consumer);
}
// A block's LAST conv writes only the bf16 input copy of its pool ("pool<b>in"): the pool is its only reader, and pool1 / pool2 / pool5 are read by
// bf16 convolutions only (consumer: the next block's first conv, or fc6).
inline bool pool_in_bf16(const Bf16Opts& o, const ConvShape& last, const ConvShape& consumer, int block)
{
    return o.copies && o.acts && o.fuse_pool && !pool_feeds_skip(block) && bf16_kernels_take(last) && bf16_kernels_take(consumer);
}
// -- forward: a block's pool --
// the pool keeps its routing bytes (the backward pass reads one byte per window instead of the block's last activation)
inline bool pool_routes(const Bf16Opts& o, const ConvShape& last) { return o.copies && o.fuse_pool && bf16_kernels_take(last); }
// ... and writes its consumer's padded bf16 input copy itself
inline bool pool_out_bf16(const Bf16Opts& o, const ConvShape& last, const ConvShape& consumer) { return pool_routes(o, last) && o.acts && bf16_kernels_take(consumer); }
// ... as the output's only form (no fp32 pool tensor)
inline bool pool_out_bf16_only(const Bf16Opts& o, const ConvShape& last, const ConvShape& consumer, int block)
{
    return pool_out_bf16(o, last, consumer) && !pool_feeds_skip(block);
}
// ... from the last conv's bf16 copy (pool_in_bf16): that kernel has no fp32 output, so exactly where the output is bf16 only.  The rule's half;
// the site adds the run-time half -- the copy exists and this pass filled it.
inline bool pool_reads_bf16(const Bf16Opts& o, const ConvShape& last, const ConvShape& consumer, int block) { return pool_out_bf16_only(o, last, consumer, block); }
// -- forward: fc6 / fc7 --  fc7's padded input copy comes out of fc6's epilogue (else: a conversion pass of fc6's fp32 output)
inline bool fc7_in_from_fc6(const Bf16Opts& o) { return o.copies && o.acts; }

// -- backward --
// Layer l's output gradient exists only as its padded bf16 copy: the data gradient of `producer` (the next conv on l's map) writes the copy and
// l's bias gradient instead of the fp32 tensor.  Both gradients of l then read the copy: never conv1_1, whose weight gradient is exact fp32 and
// reads the fp32 tensor.  backward_blocks asks, conv_dgrad acts on it (DgradEpi::yb_only).
inline bool dy_bf16_only(const Bf16Opts& o, const ConvShape& l, bool l_is_conv1_1, const ConvShape& producer)
{
    return o.acts && !l_is_conv1_1 && l.K == 3 && producer.K == 3 && bf16_kernels_take(l) && bf16_kernels_take(transposed(l)) && bf16_kernels_take(transposed(producer));
}
// The pool's backward kernel writes the bf16 dZ copy and the bias gradient of the block's last conv and no fp32 dZ: both of that conv's gradients
// take the copy (Cin == Cout: see the precondition).  backward_blocks asks.
inline bool pool_bwd_writes_bf16(const Bf16Opts& o, const ConvShape& last) { return o.fuse_pool && bf16_kernels_take(last); }

}  // namespace fcn8s
