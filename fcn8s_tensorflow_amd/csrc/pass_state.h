// What a forward or backward pass of fcn8s_model left behind for the launches that follow it (m->pass), and the four places its lifetimes end.
// Host-only C++ (no HIP include): tests/test_pass_state_host.py builds it with a plain compiler.  Keys are layer names ("conv3_2", "fc6", ...).
#pragma once
#include <set>
#include <string>

namespace fcn8s {

// One slot: "a scratch buffer holds some quantity of layer L, for whoever asks next".  The buffer and the quantity are the slot's meaning
// (see PassState); the slot only remembers L.
struct Handoff {
    void give(const char* layer) { who = layer ? layer : ""; }            // over a full slot: the buffer was rewritten, the older promise is gone
    bool holds(const char* layer) const { return layer && !who.empty() && who == layer; }
    bool take(const char* layer) { const bool mine = holds(layer); if (mine) who.clear(); return mine; }      // true exactly once; another layer's slot stays
    void drop() { who.clear(); }
private:
    std::string who;
};

struct PassState {
    using Layers = std::set<std::string>;

    // ---- forward facts: what the last forward pass did, read by that pass's later layers, by the backward pass and by fcn8s_get_activation
    Layers rbits_ok;                 // layers whose ReLU bit mask ("rb:<layer>") this pass wrote
    Layers y_unwritten;              // layers whose activation tensor this pass did not materialise
    Layers in_bf16_only;             // bf16_train, option bf16_acts: layers whose fp32 INPUT was not written (their padded bf16 copy is all there is)
    Layers xg16_filled;              // bf16_train: input copies (xg16) a producing kernel's epilogue has already written (no conversion pass)
    Layers q8_filled;                // fp8_infer: e4m3 input copies (q8) written by this pass
    bool pool_fused[5] = {};         // block b's pool + argmax bytes came out of conv_b_last's output transform (or a routing pool stood in for it)
    bool pool_routed[5] = {};        // bf16_train: block b's pool kept its routing bytes (pidx<b>) for maxpool_bwd_bf16_route_kernel
    Handoff fft6_ready;              // the layer whose DFT filter bank (u_train "<layer>#fft") this pass built; the data gradient asks with holds()
    Handoff fft6_xf;                 // "wv:<layer>" holds the DFT input bank Xf of the layer: taken by its weight gradient

    // ---- backward facts: what this backward pass has done so far
    Layers dyg16_filled;             // bf16_train: output-gradient copies (dyg16) already written by their producer
    Layers db_taken;                 // layers whose bias gradient the producer of their dY copy has already added
    Layers dy_bf16_only;             // layers whose fp32 OUTPUT GRADIENT was not written (their padded bf16 copy + the bias gradient were)
    Layers dz_unwritten;             // layers whose fp32 dY the pool's backward kernel skipped

    // ---- hand-offs through the shared Winograd / DFT scratch
    Handoff fwd_v;                   // forward: the layer's V is written (by the previous conv's fused output transform, or conv1_1's gather): no input transform
    Handoff dgrad_v;                 // d_wino_v holds the input transform of the layer's data gradient (its weight gradient's fused transform wrote it)
    Handoff dm;                      // d_wino_m holds the layer's dM = A dY A^T (its weight gradient left it): the adjoint data gradient reads it
    Handoff dm_prefilled;            // d_wino_m holds the layer's dM INSTEAD of its dZ (the next layer's data gradient wrote it): its weight gradient must take it
    Handoff fft6_dyf;                // d_wino_m holds the layer's dYf (its DFT-domain weight gradient left it): its DFT data gradient takes it

    // forward() before its first launch.  q8_filled belongs to fp8 passes alone: every other pass leaves the e4m3 copies of the last fp8 pass as they
    // are (fcn8s_get_activation("q8:...") still describes that pass).  pool_fused / pool_routed had no clearing line before: forward() assigns all five
    // of each before it returns, and after a pass that failed half way the backward pass is undefined with or without them: no reader sees the difference.
    void begin_forward(bool fp8_pass)
    {
        rbits_ok.clear(); y_unwritten.clear(); in_bf16_only.clear(); xg16_filled.clear();
        if (fp8_pass) q8_filled.clear();
        for (int b = 0; b < 5; ++b) pool_fused[b] = pool_routed[b] = false;
        fft6_ready.drop(); fft6_xf.drop(); fft6_dyf.drop(); fwd_v.drop();       // (fft6_dyf: the dYf of a pass before)
    }
    // Bucket 0 of a backward pass.  Of the hand-offs only dm_prefilled goes: a leftover (a pass that ended in an error between the promise and its
    // weight gradient) would raise an error in this pass.  dm and dgrad_v are voided by the pass's first convolution (drop_backward_handoffs).
    void begin_backward() { dyg16_filled.clear(); db_taken.clear(); dy_bf16_only.clear(); dz_unwritten.clear(); dm_prefilled.drop(); }
    // The padded copies lost their contents (drop_shape_copies): another shape, or the copies are gone.  keep_regrowable: the q8 copies stay and
    // re-border themselves, so what the last fp8 pass filled stays recorded.
    void forget_shape_copies(bool keep_regrowable)
    {
        xg16_filled.clear(); dyg16_filled.clear();
        if (!keep_regrowable) q8_filled.clear();
    }
    // d_wino_v / d_wino_m belong to whichever convolution runs next: any convolution launched between a weight gradient and its own data
    // gradient voids the dM / V that weight gradient left.  (dm_prefilled and fft6_dyf have exactly one taker each and are dropped there.)
    void drop_backward_handoffs() { dm.drop(); dgrad_v.drop(); }
};

}  // namespace fcn8s
