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

}  // namespace fcn8s
